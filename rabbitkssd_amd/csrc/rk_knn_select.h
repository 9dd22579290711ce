// rk_knn_select.h -- the CSR adjacency of the keyed records and the wave64 selection of a genome's k nearest records (not part of the
// public ABI): what rk_knn.hip (k_knn_select: the first k records of every genome) and rk_mreach.hip (k_mreach_core: the k-th alone)
// run behind rk_edge_stage.h's key pass and k_edge_degree.  DESIGN.md 4.9.
//
//   offsets   k_knn_offsets writes min(deg, k) and the largest degree; an exclusive scan of deg[] gives the adjacency offsets aoff[];
//   fill      k_knn_fill: per live record and endpoint v the 16-byte entry {w, other << 32 | e} at aoff[v] + atomicAdd(cur + v, 1).
//             Entries compared as (first word, second word) ascending are the order of a genome's list: the ratio descending, exactly,
//             then the neighbour's caller index (e < 2^31: more records fall back).  The place inside a segment depends on the run,
//             the selection's result does not;
//   select    knn_select_wave: one wave64 per genome.  Lane l holds the l-th best entry so far or (kDead, kDead); lanes >= k stay dead.
//             The segment streams in chunks of 64, one 16-byte load per lane; a ballot keeps the candidates that beat the current k-th
//             (lane k - 1); each survivor is broadcast, tested again against the tightened k-th, ranked by the number of lanes that
//             precede it and inserted with one shuffle up.  No barrier: the waves of a workgroup have different trip counts.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rk_edge_order.h"
#include "rk_edge_stage.h"

namespace {

constexpr uint32_t kKnnDeviceMax = 64;   // one list slot per lane of a wave64
constexpr uint32_t kWave = 64;

struct __align__(16) KnnEntry {
    unsigned long long w, x;   // ~ratio key; neighbour << 32 | record number
};

// kmin[i] = min(deg[i], k); deg[N] is 0 (the scans then end in the totals); *max_deg: one atomic per wave
__global__ void __launch_bounds__(kStageThreads)
k_knn_offsets(const uint32_t *deg, uint32_t *kmin, uint32_t n, uint32_t k, uint32_t *max_deg)
{
    uint32_t most = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
        const uint32_t d = deg[i];
        kmin[i] = min(d, k);
        most = max(most, d);
    }
    for (int d = warpSize / 2; d > 0; d >>= 1) most = max(most, (uint32_t)__shfl_down(most, d));
    if ((threadIdx.x & (warpSize - 1)) == 0 && most) atomicMax(max_deg, most);
}

// aoff[v] + cur[v] stays below aoff[v + 1]: the degree pass counted the same live records
__global__ void __launch_bounds__(kStageThreads)
k_knn_fill(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *aoff, uint32_t *cur, KnnEntry *adj)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t a = (uint32_t)(p >> 32), b = (uint32_t)p;
        adj[(unsigned long long)aoff[a] + atomicAdd(cur + a, 1u)] = KnnEntry{we, ((unsigned long long)b << 32) | e};
        adj[(unsigned long long)aoff[b] + atomicAdd(cur + b, 1u)] = KnnEntry{we, ((unsigned long long)a << 32) | e};
    }
}

__device__ __forceinline__ bool entry_less(unsigned long long aw, unsigned long long ax, unsigned long long bw, unsigned long long bx)
{
    return aw < bw || (aw == bw && ax < bx);
}

// the value lane `src` holds, src the same in every lane: two scalar reads, nothing through the LDS crossbar
__device__ __forceinline__ unsigned long long lane_value(unsigned long long v, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// The first k entries of adj[beg .. end) in order, entry l in lane l as (*best_w, *best_x); (kDead, kDead) in the lanes beyond them.
// 1 <= k <= 64.  Everything the loops branch on is the same in all lanes of a wave (beg, end, ballots, broadcasts).
__device__ __forceinline__ void knn_select_wave(const KnnEntry *adj, unsigned long long beg, unsigned long long end, uint32_t lane, uint32_t k,
                                                unsigned long long *best_w, unsigned long long *best_x)
{
    const int kth = (int)k - 1;
    unsigned long long bw = kDead, bx = kDead;   // lane l: the l-th best entry so far
    for (unsigned long long at = beg; at < end; at += kWave) {
        unsigned long long cw = kDead, cx = kDead;
        if (at + lane < end) {
            const KnnEntry c = adj[at + lane];
            cw = c.w;
            cx = c.x;
        }
        unsigned long long mask = __ballot(entry_less(cw, cx, lane_value(bw, kth), lane_value(bx, kth)));
        while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const unsigned long long sw = lane_value(cw, src), sx = lane_value(cx, src);
            if (!entry_less(sw, sx, lane_value(bw, kth), lane_value(bx, kth))) continue;   // an earlier survivor tightened the k-th
            const uint32_t rank = (uint32_t)__popcll(__ballot(entry_less(bw, bx, sw, sx)));   // < k: lane k - 1 does not precede it
            const unsigned long long uw = __shfl_up(bw, 1), ux = __shfl_up(bx, 1);
            if (lane < k && lane >= rank) {
                bw = lane == rank ? sw : uw;
                bx = lane == rank ? sx : ux;
            }
        }
    }
    *best_w = bw;
    *best_x = bx;
}

}  // namespace
