// rk_edge_order.h -- the order of hit records by nearness (not part of the public ABI): the keys of rk_edge_stage.h's key pass and of
// the kernels of rk_forest.hip, rk_greedy.hip, rk_knn.hip and rk_mreach.hip that follow it, and the exact order of their host sides.
//
// Order of edges (include/rabbitkssd.h, clusters section): the ratio common / u descending -- u = size0 + size1 - common (metric 0)
// or min(size0, size1) (metric 1); both distances fall strictly as it rises --, then row ascending, then col ascending.  On the
// device the ratio is the 64-bit key floor(common * 2^62 / u), exact for 0 < common <= u < 2^31 (distinct fractions differ by more
// than 2^-62); `w` = ~key turns "nearest first" into an unsigned minimum.  On the host the ratios are compared by cross-multiplication.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rabbitkssd.h"

namespace {

constexpr unsigned long long kDead = ~0ULL;  // w of a record that takes no part (any more)

// common / u of a record as signed 64-bit terms (u may be <= 0 only for multisets whose counts are products of multiplicities)
__host__ __device__ inline void ratio_terms(int32_t common, int32_t size0, int32_t size1, int metric, long long *c, long long *u)
{
    *c = common;
    *u = metric ? (long long)(size0 < size1 ? size0 : size1) : (long long)size0 + size1 - common;
}

// floor(c * 2^62 / u) for 0 < c <= u < 2^31 in two division steps of 31 bits: every intermediate stays below 2^62
__device__ __forceinline__ unsigned long long ratio_key(unsigned long long c, unsigned long long u)
{
    const unsigned long long q1 = (c << 31) / u, r1 = (c << 31) % u;
    return (q1 << 31) | ((r1 << 31) / u);
}

__device__ __forceinline__ void min_u64(unsigned long long *p, unsigned long long v)
{
    // the load saves the atomic of a record that cannot win (the values only fall: a stale one costs an atomic, nothing else)
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- host: the order of edges, exactly ------------------------------------------------------------------------------------
// ratio descending by cross-multiplication (128-bit: u reaches 2^32), then row, then col.  A record without a ratio (u <= 0 or
// common < 0: no join reports one) comes behind every record that has one.
struct EdgeLess {
    int metric;
    bool operator()(const rk_hit &a, const rk_hit &b) const
    {
        long long ca, ua, cb, ub;
        ratio_terms(a.common, a.size0, a.size1, metric, &ca, &ua);
        ratio_terms(b.common, b.size0, b.size1, metric, &cb, &ub);
        const bool va = ua > 0 && ca >= 0, vb = ub > 0 && cb >= 0;
        if (va != vb) return va;
        if (va) {
            const __int128 l = (__int128)ca * ub, r = (__int128)cb * ua;
            if (l != r) return l > r;
        }
        return a.row != b.row ? a.row < b.row : a.col < b.col;
    }
};

inline uint32_t other_end(const rk_hit &h, uint32_t v) { return h.row == v ? h.col : h.row; }

// the order of genome v's list (rk_knn_rows, the core record of rk_mreach_rows): EdgeLess with the endpoint v fixed -- ratio first,
// then the neighbour's index
struct NeighbourLess {
    int metric;
    uint32_t v;
    bool operator()(const rk_hit &a, const rk_hit &b) const
    {
        rk_hit x = a, y = b;
        x.row = y.row = 0;
        x.col = other_end(a, v);
        y.col = other_end(b, v);
        return EdgeLess{metric}(x, y);
    }
};

}  // namespace
