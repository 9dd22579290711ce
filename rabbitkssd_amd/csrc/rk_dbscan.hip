// rk_dbscan.hip -- density-based clusters (DBSCAN) of `alldist` on the device (rk_dbscan_rows) and the same rule on the host over a hit
// list the caller already has (rk_dbscan_hits).  The graph is that of rk_cluster_rows.  deg(v) = the records incident to v; v is CORE
// iff deg(v) + 1 >= min_pts (min_pts counts the genome itself); clusters are the components of the subgraph induced by the core
// genomes, labelled by their smallest core index; a non-core genome with a core neighbour is BORDER and takes the label of its nearest
// core neighbour (order of rk_edge_order.h restricted to it: ratio descending, exactly, then the neighbour's caller index); every
// other genome is NOISE.  include/rabbitkssd.h, density-based clusters.
//
//   stage     rk_edge_stage.h: the self join into a device buffer, its key pass (EdgeStage::key_pass<true>: per record w and
//             row << 32 | col; a BORDERLINE record goes, with its slot number, to the small host buffer and is dead for now; a record
//             outside 0 < common <= u -- multisets -- is counted: the call refuses such a collection), the two retries;
//   host      the stage decides the borderline records BEFORE any degree is counted (one kept edge can make a genome core and merge
//             two clusters arbitrarily far away); the slot numbers of the kept ones go back up and k_edge_revive gives them their keys;
//   degree    k_edge_degree: per live record one atomicAdd on deg[row] and one on deg[col];
//   hook      k_dbscan_hook, one sweep: both endpoints core -> p_link(parent, row, col); exactly one core -> the atomic minimum of w
//             at the other endpoint (best_w);
//   border    k_dbscan_border, one sweep: exactly one endpoint core and w == best_w[the other] -> the atomic minimum of the core
//             endpoint's index there (best_nb).  Two steps because the key is 64 + 32 bits; no third, because nothing but the
//             neighbour's index is kept;
//   labels    k_dbscan_labels, per genome: kind, label (the settled root of the genome itself, or of best_nb for a border genome), via,
//             and wave-reduced counts of the kinds and of the roots;
//   host      labels, via, degrees, kinds and the counters are the tail of the stage's counter block: one read-back of 13 * N + 32
//             bytes, never O(hits).
//
// Memory scope: w[], rc[], deg[], best_w[], best_nb[] and parent[] are written by one kernel and read by a later one on the same stream
// (plain accesses behind kernel boundaries: the hook reads deg[] plainly, the border sweep best_w[], the label pass parent[] and
// best_nb[] through p_settled_root).  Inside k_dbscan_hook parent[] is touched only through rk_union_find.h's agent-scope relaxed
// atomics (the eight XCDs have L2s of their own); the only other communication inside a kernel is the two relaxed agent-scope minima
// (values only fall, the minimum does not depend on arrival order) and the atomic adds of the degree and the counters.
// Termination: only core genomes are ever linked, parent[x] <= x at every moment and a root is only ever linked under a smaller index:
// every chain strictly decreases, a failed compare-and-swap has observed a strictly smaller parent, and a root is the
// smallest core index of its cluster.  No loop waits for another workgroup, there are no barriers: any grid works.  DESIGN.md 4.10.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_edge_order.h"
#include "rk_union_find.h"
#include "rk_edge_stage.h"

namespace {

constexpr uint32_t kNoise = RK_DBSCAN_NOISE;
enum : uint8_t { kKindNoise = 0, kKindBorder = 1, kKindCore = 2 };
// the counters in front of the results in the stage's tail (u64 each)
enum { kOutClusters = 0, kOutCore = 1, kOutBorder = 2, kOutNoise = 3, kOutWords = 4 };

// where the results of n genomes lie in the tail: counters, then labels, via and degrees (u32 each), then kinds (u8)
struct Tail {
    unsigned long long *counts;
    uint32_t *label, *via, *deg;
    uint8_t *kind;
    Tail(void *base, uint32_t n)
        : counts((unsigned long long *)base), label((uint32_t *)(counts + kOutWords)), via(label + n), deg(via + n), kind((uint8_t *)(deg + n)) {}
    static size_t bytes(uint32_t n) { return kOutWords * 8 + (size_t)n * 13; }
};

__device__ __forceinline__ bool is_core(const uint32_t *deg, uint32_t x, uint32_t min_pts)
{
    return deg[x] >= min_pts - 1;   // deg + 1 >= min_pts, min_pts >= 1
}

__global__ void k_dbscan_init(uint32_t *parent, unsigned long long *best_w, uint32_t *best_nb, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        parent[i] = i;
        best_w[i] = kDead;
        best_nb[i] = kNoise;
    }
}

// deg[] is final: written by k_edge_degree, a kernel boundary away
__global__ void __launch_bounds__(kStageThreads)
k_dbscan_hook(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *deg, uint32_t min_pts, uint32_t *parent,
              unsigned long long *best_w)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t a = (uint32_t)(p >> 32), b = (uint32_t)p;
        const bool ca = is_core(deg, a, min_pts), cb = is_core(deg, b, min_pts);
        if (ca && cb) p_link(parent, a, b);
        else if (ca != cb) min_u64(best_w + (ca ? b : a), we);
    }
}

// best_w[] is final: among the records that match it the smallest core neighbour wins
__global__ void __launch_bounds__(kStageThreads)
k_dbscan_border(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *deg, uint32_t min_pts,
                const unsigned long long *best_w, uint32_t *best_nb)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t a = (uint32_t)(p >> 32), b = (uint32_t)p;
        const bool ca = is_core(deg, a, min_pts), cb = is_core(deg, b, min_pts);
        if (ca == cb) continue;
        const uint32_t core = ca ? a : b, other = ca ? b : a;
        if (best_w[other] == we) __hip_atomic_fetch_min(best_nb + other, core, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// parent[] and best_nb[] are final.  counts: one atomic per wave and counter
__global__ void __launch_bounds__(kStageThreads)
k_dbscan_labels(const uint32_t *deg, const uint32_t *parent, const uint32_t *best_nb, uint32_t min_pts, uint32_t n, uint32_t *label, uint32_t *via,
                uint8_t *kind, unsigned long long *counts)
{
    uint32_t seen[kOutWords] = {0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t l = kNoise, v = kNoise;
        uint8_t k = kKindNoise;
        if (is_core(deg, i, min_pts)) {
            k = kKindCore;
            l = p_settled_root(parent, i);
            seen[kOutCore]++;
            seen[kOutClusters] += l == i;
        } else if (best_nb[i] != kNoise) {
            k = kKindBorder;
            v = best_nb[i];
            l = p_settled_root(parent, v);
            seen[kOutBorder]++;
        } else seen[kOutNoise]++;
        label[i] = l;
        via[i] = v;
        kind[i] = k;
    }
    for (int c = 0; c < kOutWords; c++) {
        uint32_t s = seen[c];
        for (int d = warpSize / 2; d > 0; d >>= 1) s += __shfl_down(s, d);
        if ((threadIdx.x & (warpSize - 1)) == 0 && s) atomicAdd(counts + c, (unsigned long long)s);
    }
}

struct Result {
    std::vector<uint32_t> label, via, deg;
    std::vector<uint8_t> kind;
    uint32_t n_clusters = 0, n_core = 0, n_border = 0, n_noise = 0;
};

// the rule over a hit list (validated by the caller)
void dbscan_of_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t min_pts, int metric, Result *r)
{
    std::vector<uint64_t> start, adj;
    hit_adjacency(hits, n_hits, n, &start, &adj);
    r->label.assign(n, kNoise);
    r->via.assign(n, kNoise);
    r->deg.resize(n);
    r->kind.assign(n, kKindNoise);
    for (uint32_t v = 0; v < n; v++) {
        r->deg[v] = (uint32_t)(start[v + 1] - start[v]);
        if ((uint64_t)r->deg[v] + 1 >= min_pts) r->kind[v] = kKindCore;
    }
    std::vector<uint32_t> parent(n);
    for (uint32_t v = 0; v < n; v++) parent[v] = v;
    for (uint64_t e = 0; e < n_hits; e++)
        if (r->kind[hits[e].row] == kKindCore && r->kind[hits[e].col] == kKindCore) host_union(parent.data(), hits[e].row, hits[e].col);
    host_flatten(parent.data(), n);
    const EdgeLess nearer{metric};
    for (uint32_t v = 0; v < n; v++) {
        if (r->kind[v] == kKindCore) {
            r->label[v] = parent[v];
            r->n_core++;
            r->n_clusters += parent[v] == v;
            continue;
        }
        rk_hit best{};
        for (uint64_t at = start[v]; at < start[v + 1]; at++) {
            const rk_hit &h = hits[adj[at]];
            const uint32_t other = h.row == v ? h.col : h.row;
            if (r->kind[other] != kKindCore) continue;
            rk_hit x = h;   // ratio first, then the core neighbour's index
            x.row = 0;
            x.col = other;
            if (r->via[v] == kNoise || nearer(x, best)) {
                best = x;
                r->via[v] = other;
            }
        }
        if (r->via[v] == kNoise) r->n_noise++;
        else {
            r->kind[v] = kKindBorder;
            r->label[v] = parent[r->via[v]];
            r->n_border++;
        }
    }
}

void hand_over(const Result &r, uint32_t n, uint32_t *labels_out, uint8_t *kind_out, uint32_t *via_out, uint32_t *degree_out)
{
    if (!n) return;
    memcpy(labels_out, r.label.data(), (size_t)n * 4);
    memcpy(kind_out, r.kind.data(), n);
    if (via_out) memcpy(via_out, r.via.data(), (size_t)n * 4);
    if (degree_out) memcpy(degree_out, r.deg.data(), (size_t)n * 4);
}

}  // namespace

extern "C" {

int rk_dbscan_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t min_pts, int metric, uint32_t *labels_out, uint8_t *kind_out,
                   uint32_t *via_out, uint32_t *degree_out)
{
    if ((n_hits && !hits) || (n && (!labels_out || !kind_out)) || !min_pts) return RK_ERR_ARG;
    for (uint64_t e = 0; e < n_hits; e++)
        if (hits[e].row >= n || hits[e].col >= n || hits[e].row == hits[e].col) return RK_ERR_ARG;
    Result r;
    dbscan_of_hits(hits, n_hits, n, min_pts, metric != 0, &r);
    hand_over(r, n, labels_out, kind_out, via_out, degree_out);
    return RK_OK;
}

int rk_dbscan_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t min_pts, uint32_t *labels_out, uint8_t *kind_out,
                   uint32_t *via_out, uint32_t *degree_out, rk_dbscan_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_dbscan_stats st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    const uint32_t N = idx->n_ref;
    if (N && (!labels_out || !kind_out)) return rk_fail(ctx, RK_ERR_ARG, "labels_out or kind_out is null");
    if (!min_pts) return rk_fail(ctx, RK_ERR_ARG, "rk_dbscan_rows: min_pts counts the genome itself and must be 1 or more");
    const StageNeeds needs{"rk_dbscan_rows", "the degrees of a row shard are partial, and the core test does not compose from shards", true};
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    if (!N) return RK_OK;
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
    const TimedSpan span{ctx, RK_MS_DBSCAN};
    span.clear();

    // the same rule over the hit list on the host: the A/B leg of tools/dbscan_probe.py, and a fallback
    if (rk_switched_off("RK_DBSCAN_DEVICE")) {
        rk_hit *hits = nullptr;
        uint64_t n_hits = 0;
        if (int rc = rk_dist_rows(ctx, idx, nullptr, opts, &hits, &n_hits, nullptr)) return rc;
        Result r;
        dbscan_of_hits(hits, n_hits, N, min_pts, opts->metric != 0, &r);
        rk_free_host(hits);
        hand_over(r, N, labels_out, kind_out, via_out, degree_out);
        st.edges = n_hits;
        st.n_clusters = r.n_clusters;
        st.n_core = r.n_core;
        st.n_border = r.n_border;
        st.n_noise = r.n_noise;
        if (stats) *stats = st;
        return RK_OK;
    }

    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassGreedyKeys, Tail::bytes(N));   // with slot numbers; the tail: the results
    stage.tail_in_pass = false;   // (the key pass writes none of them)
    DevBuf<unsigned long long> w(ctx), rc_(ctx), best_w(ctx);
    DevBuf<uint32_t> parent(ctx), best_nb(ctx);
    RK_HIP(ctx, parent.alloc(N));
    RK_HIP(ctx, best_w.alloc(N));
    RK_HIP(ctx, best_nb.alloc(N));

    // the key pass: nothing is counted before the stage is through
    int rc = stage.run([&](int pass) { return stage.key_pass<true>(pass, w, rc_); });
    if (rc) return rc;
    stage.stats(&st);
    // the borderline records, decided before any degree
    if ((rc = stage.revive(w.p, &st.borderline_kept))) return rc;
    const unsigned long long n_rec = stage.n_hits;
    const unsigned grid = grid_for(ctx, n_rec), vgrid = grid_for(ctx, N);
    const Tail out(stage.tail(), N);
    RK_HIP(ctx, hipMemsetAsync(out.counts, 0, kOutWords * 8, stream));
    RK_HIP(ctx, hipMemsetAsync(out.deg, 0, (size_t)N * 4, stream));
    hipLaunchKernelGGL(k_dbscan_init, dim3(vgrid), dim3(kStageThreads), 0, stream, parent.p, best_w.p, best_nb.p, N);
    hipLaunchKernelGGL(k_edge_degree, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, out.deg);
    RK_HIP(ctx, hipGetLastError());
    RK_HIP(ctx, span.begin());
    hipLaunchKernelGGL(k_dbscan_hook, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, out.deg, min_pts, parent.p, best_w.p);
    hipLaunchKernelGGL(k_dbscan_border, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, out.deg, min_pts, best_w.p, best_nb.p);
    hipLaunchKernelGGL(k_dbscan_labels, dim3(vgrid), dim3(kStageThreads), 0, stream, out.deg, parent.p, best_nb.p, min_pts, N, out.label, out.via, out.kind,
                       out.counts);
    RK_HIP(ctx, hipGetLastError());
    RK_HIP(ctx, span.end());
    if ((rc = stage.fetch_home())) return rc;
    span.read();
    const Tail home((void *)stage.home_tail(), N);
    if (home.counts[kOutCore] + home.counts[kOutBorder] + home.counts[kOutNoise] != N || home.counts[kOutClusters] > home.counts[kOutCore])
        return rk_fail(ctx, RK_ERR_HIP, "rk_dbscan_rows: the kinds of %u genomes do not add up (internal error)", N);
    memcpy(labels_out, home.label, (size_t)N * 4);
    memcpy(kind_out, home.kind, N);
    if (via_out) memcpy(via_out, home.via, (size_t)N * 4);
    if (degree_out) memcpy(degree_out, home.deg, (size_t)N * 4);
    st.n_clusters = (uint32_t)home.counts[kOutClusters];
    st.n_core = (uint32_t)home.counts[kOutCore];
    st.n_border = (uint32_t)home.counts[kOutBorder];
    st.n_noise = (uint32_t)home.counts[kOutNoise];
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
