// rk_boruvka.h -- the Boruvka rounds over keyed hit records (not part of the public ABI): what rk_forest.hip (w = ~ratio key) and
// rk_mreach.hip (w = the mutual-reachability weight) run behind rk_edge_stage.h's key pass, and the Kruskal of their host sides.
//
//   rounds    k_forest_match_w (atomic minimum of w per component, both endpoints), k_forest_match_rc (among the records that match
//             that w, atomic minimum of row << 32 | col), k_forest_link (a record that is the best edge of either of its components
//             is appended once to the forest buffer -- with its w beside it where the caller asks for that --, its roots linked with
//             the compare-and-swap hook), k_forest_flatten (label[i] = root(i), best arrays reset).  The host reads one counter per
//             round and stops when a round appended nothing.
//
// Termination and acyclicity: DESIGN.md 4.7.  In short: the order (w, row, col) is strict whatever w is -- ties in w are broken by the
// pair, and a pair has one record --, so the best edges of one round form a forest over the round's components (a cycle would need an
// edge that is smaller than itself), apart from the edge both of its components chose, which is ONE record and whose single thread
// appends it once.  Hence every k_forest_link thread unites two different trees, whatever the others do meanwhile, and its
// compare-and-swap loop ends as k_cluster_hook's does.  No loop waits for another workgroup.
// Memory scope: label[] and the best arrays are written by one kernel and read by the next (plain loads behind the kernel boundary;
// the minima themselves are agent-scope atomics); parent[] inside k_forest_link only through agent-scope relaxed atomics.
#pragma once
#include <numeric>
#include <vector>

#include "rk_edge_order.h"
#include "rk_edge_stage.h"
#include "rk_union_find.h"

namespace {

__global__ void k_forest_init(uint32_t *parent, uint32_t *label, unsigned long long *best_w, unsigned long long *best_rc, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        parent[i] = i;
        label[i] = i;
        best_w[i] = kDead;
        best_rc[i] = kDead;
    }
}

// (In the kernels of the rounds n_hits_dev counts every hit of the join, those beyond `cap` included: they read what was written.)
// label[] is the round's start: written by k_forest_flatten / k_forest_init, a kernel boundary away.  A record inside one component
// stays inside it: dead from here on (its own thread is the only one that touches w[e]).
__global__ void __launch_bounds__(kStageThreads)
k_forest_match_w(unsigned long long *w, const unsigned long long *rc, const unsigned long long *n_hits_dev, unsigned long long cap,
                 const uint32_t *label, unsigned long long *best_w)
{
    const unsigned long long n_rec = min(*n_hits_dev, cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t la = label[(uint32_t)(p >> 32)], lb = label[(uint32_t)p];
        if (la == lb) {
            w[e] = kDead;
            continue;
        }
        min_u64(best_w + la, we);
        min_u64(best_w + lb, we);
    }
}

__global__ void __launch_bounds__(kStageThreads)
k_forest_match_rc(const unsigned long long *w, const unsigned long long *rc, const unsigned long long *n_hits_dev, unsigned long long cap,
                  const uint32_t *label, const unsigned long long *best_w, unsigned long long *best_rc)
{
    const unsigned long long n_rec = min(*n_hits_dev, cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t la = label[(uint32_t)(p >> 32)], lb = label[(uint32_t)p];
        if (best_w[la] == we) min_u64(best_rc + la, p);
        if (best_w[lb] == we) min_u64(best_rc + lb, p);
    }
}

// la and lb are the roots of the record's trees at the round's start, so the walk to today's roots starts there
__global__ void __launch_bounds__(kStageThreads)
k_forest_link(const rk_hit *hits, unsigned long long *w, const unsigned long long *rc, const unsigned long long *n_hits_dev, unsigned long long cap,
              const uint32_t *label, const unsigned long long *best_w, const unsigned long long *best_rc, uint32_t *parent, rk_hit *forest,
              unsigned long long forest_cap, unsigned long long *n_forest, unsigned long long *forest_w = nullptr)
{
    const unsigned long long n_rec = min(*n_hits_dev, cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t la = label[(uint32_t)(p >> 32)], lb = label[(uint32_t)p];
        const bool best = (best_w[la] == we && best_rc[la] == p) || (best_w[lb] == we && best_rc[lb] == p);
        if (!best) continue;
        const unsigned long long at = atomicAdd(n_forest, 1ULL);
        if (at < forest_cap) {   // (a forest has at most N - 1 edges; the host checks the counter)
            forest[at] = hits[e];
            if (forest_w) forest_w[at] = we;   // (where w is not a function of the record alone)
        }
        w[e] = kDead;
        p_link(parent, la, lb);
    }
}

__global__ void k_forest_flatten(const uint32_t *parent, uint32_t *label, unsigned long long *best_w, unsigned long long *best_rc, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        label[i] = p_settled_root(parent, i);
        best_w[i] = kDead;
        best_rc[i] = kDead;
    }
}

// Kruskal over edges that are in order already: the accepted ones, in order, compacted to the front.  Returns their number.
uint64_t kruskal_sorted(rk_hit *e, uint64_t m, uint32_t n)
{
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    uint64_t k = 0;
    for (uint64_t i = 0; i < m; i++)
        if (host_union(parent.data(), e[i].row, e[i].col)) {
            if (k != i) e[k] = e[i];
            k++;
        }
    return k;
}

}  // namespace
