// rk_query_dev.h -- the device side that the consumers of query sketches share (rk_mask.hip, rk_lca.hip, rk_screen.hip, rk_gather.hip;
// not part of the public ABI), one definition each.  The host side is rk_query_host.h.  DESIGN.md 4.19.
//
//   wave      relaxed agent-scope adds, 64-bit shuffles, the lanes below a lane, a wave's sum, and the wave-aggregated reservations
//             (queue_slot, wave_append: ONE atomic per wave).  rk_group.hip takes these too, rk_assign.hip and rk_medoid.hip the adds;
//   look-up   index_lookup: the posting list of a query hash -- the bucket of the prefix directory, then a binary search among the
//             distinct hashes of the index, the kTrips searches of a lane advancing together (one probe of each per step: the loads of
//             a step are in flight at once).  k_mask_flag and k_lca_tally run it with 8 trips, k_screen_win with 4, k_gather_match
//             with 1.  index_lookup_of fills its arguments from an index;
//   prepare   k_query_prepare: the sketch sizes (and the internal ids) by the CALLER's reference index, once per call;
//   scan      k_query_scan: one workgroup, an exclusive scan in 64 bits of per-row counts into the rows' regions.
#pragma once
#include <cstdint>

#include "rk_internal.h"

namespace {

// ---- wave helpers: every lane of a full wave calls the collective ones in converged code --------------------------------------
__device__ __forceinline__ unsigned long long add_u64(unsigned long long *p, unsigned long long v)
{
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_u32(uint32_t *p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
    return ((unsigned long long)hi << 32) | lo;
}
// the bits of the lanes below `lane` (0 .. 63; a shift by 64 is no shift at all: lane 0 is told apart)
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return lane ? (~0ULL >> (64 - lane)) : 0ULL; }
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
    return v;
}
// a slot of a queue behind *counter for the lanes with `mine` (the others get 0): one atomic per wave
__device__ __forceinline__ uint32_t queue_slot(bool mine, unsigned long long *counter)
{
    const unsigned long long m = __ballot(mine);
    if (!m) return 0;   // (uniform)
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == lead) base = add_u64(counter, (unsigned long long)__popcll(m));
    return (uint32_t)(shfl_u64(base, lead) + (unsigned long long)__popcll(m & lanes_below(lane)));
}
// at most one entry per lane behind *counter, one atomic per wave (the counter counts past any capacity: an entry beyond it is dropped)
__device__ __forceinline__ void wave_append(bool mine, unsigned long long key, unsigned long long *counter, unsigned long long *buf, unsigned long long cap)
{
    const unsigned long long m = __ballot(mine);
    if (!m) return;   // (uniform)
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == lead) base = add_u64(counter, (unsigned long long)__popcll(m));
    const unsigned long long at = shfl_u64(base, lead) + (unsigned long long)__popcll(m & lanes_below(lane));
    if (mine && at < cap) buf[at] = key;
}

// ---- the look-up ---------------------------------------------------------------------------------------------------------------
struct IndexLookup {
    const void *uhash;        // Hash[U]: the index's distinct hashes, ascending
    const uint32_t *dir;      // u32[2^dir_bits + 1]
    unsigned long long U;     // 0: nothing is looked up
    int32_t hash_bits, dir_shift;
};

// (the directory exists: rk_index_ensure_dir, which a caller with U > 0 runs first)
inline IndexLookup index_lookup_of(const rk_index *idx)
{
    return IndexLookup{idx->wide ? (const void *)idx->d_uhash64 : (const void *)idx->d_uhash, idx->d_dir, idx->U, idx->hash_bits, idx->dir_shift};
}

constexpr uint32_t kNoList = 0xFFFFFFFFu;

// list[t] = the index of the posting list of h[t], kNoList without one (in[t] false, a hash at or beyond 2^hash_bits, U == 0)
template <class Hash, int kTrips>
__device__ __forceinline__ void index_lookup(const IndexLookup &ix, const unsigned long long (&h)[kTrips], const bool (&in)[kTrips], uint32_t (&list)[kTrips])
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

// ---- the two small kernels around a batch of rows (maybe_unused: not every file that includes this runs them) ----------------
// sizes[caller's index] = the sketch size and, with inv, inv[caller's index] = the internal id (orig == null: the identity)
[[maybe_unused]] __global__ void k_query_prepare(const uint32_t *orig, const uint32_t *sizes_internal, uint32_t n, uint32_t *inv, uint32_t *sizes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = orig ? orig[i] : i;   // (orig[] < n: rk_index_build's permutation, checked on every import of a blob)
    if (inv) inv[c] = i;
    sizes[c] = sizes_internal[i];
}

// One workgroup: off[i] = the sum of min(val[row_of[j]], limit) over j < i (row_of null: j itself; limit 0: none), off[n] = the total
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_query_scan(const uint32_t *val, const uint32_t *row_of, uint32_t n, uint32_t limit, unsigned long long *off,
                                                        unsigned long long *total_out)
{
    __shared__ unsigned long long s_wave[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long run = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += THREADS) {   // (uniform)
        const uint32_t i = c0 + tid;
        uint32_t v = 0;
        if (i < n) {
            v = val[row_of ? row_of[i] : i];
            if (limit && v > limit) v = limit;
        }
        unsigned long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long x = shfl_u64(incl, (lane - o) & 63);
            if (lane >= o) incl += x;
        }
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; k++) {
            if (k < w) before += s_wave[k];
            all += s_wave[k];
        }
        if (i < n) off[i] = run + before + incl - v;
        run += all;
        __syncthreads();   // (s_wave is rewritten by the next chunk)
    }
    if (tid == 0) {
        off[n] = run;
        if (total_out) *total_out = run;
    }
}

}  // namespace
