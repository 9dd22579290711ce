// rk_union_find.h -- the lock-free union-find over caller genome indices shared by rk_cluster.hip (k_cluster_hook) and rk_forest.hip
// (k_forest_link) on the device, the root walk of their flatten kernels, and the plain union-find of their host folds.  Invariant
// of all: parent[x] <= x, a root is only ever linked under a smaller index, so the root of a tree is its smallest member.
// Termination and memory scope of the device side: DESIGN.md 4.6.
#pragma once
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

__device__ __forceinline__ uint32_t p_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x.  Path halving: x's parent is replaced by its grandparent -- an ancestor of x, and ancestors stay ancestors
// (links are only ever added at roots), so a late or lost store costs steps, never correctness.
__device__ __forceinline__ uint32_t p_root(uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = p_load(parent + x);
        if (p == x) return x;
        const uint32_t g = p_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// unites the trees of x and y: the larger root under the smaller, with a compare-and-swap on the larger root
__device__ __forceinline__ void p_link(uint32_t *parent, uint32_t x, uint32_t y)
{
    uint32_t a = p_root(parent, x), b = p_root(parent, y);
    while (a != b) {
        const uint32_t hi = max(a, b), lo = min(a, b);
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        a = p_root(parent, seen);   // hi was linked meanwhile: seen < hi, on from there
        b = p_root(parent, lo);
    }
}

// root of x behind the kernel boundary of the last link: plain loads.  For kernels that do not write parent[], so that every
// thread walks a settled chain.
__device__ __forceinline__ uint32_t p_settled_root(const uint32_t *parent, uint32_t x)
{
    uint32_t p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

inline uint32_t host_root(uint32_t *parent, uint32_t x)
{
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

// false when a and b were in one tree already
inline bool host_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    a = host_root(parent, a);
    b = host_root(parent, b);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
    return a != b;
}

// parent[x] <= x everywhere: ascending, every parent is final before its children
inline uint32_t host_flatten(uint32_t *parent, uint32_t n)
{
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n; i++) {
        parent[i] = parent[parent[i]];
        roots += parent[i] == i;
    }
    return roots;
}
