// rk_cluster.hip -- single-linkage clusters of `alldist` on the device (rk_cluster_rows) and the host fold of two label
// arrays (rk_cluster_merge).  The users of `alldist -D d` feed its hit list into a union-find; here the components of the
// "reportable pair" graph are computed where the hit records already are: nothing of size O(hits) crosses PCIe, nothing is
// sorted, no host libm pass over the hits.
//
//   join     rk_dist_rows_dev (self join, threshold widened by 2^-46 as rk_dist_rows widens it) appends unordered hit
//            records to a device buffer of max(65,536, rows * 64) records; the counter tells an overflow (one rerun, exact);
//   k_init   parent[i] = i, indexed by the CALLER's genome index (rk_hit.row / .col carry caller indices);
//   k_hook   one grid-stride pass over the records: a record whose device distance is below D (1 - 2^-46) links the roots of
//            its two genomes, larger under smaller, with a compare-and-swap on the larger root; every other record is
//            BORDERLINE (the device's log may differ from the C library's in the last bits): appended to a small buffer for
//            the host, not linked;
//   k_flatten  label[i] = root(i) = the smallest caller index of i's component;
//   host     one read-back (two counters + N labels); borderline records decided by rk_host_exact_distances (the C
//            library's log, the reference's strict `<` of src/dist.cpp:232) and united into the labels.
//
// Termination and memory scope of k_hook: DESIGN.md 4.6.  In short: parent[x] <= x at every moment and a root is only ever
// linked under a smaller index, so every chain strictly decreases and every failed compare-and-swap has observed a strictly
// smaller parent -- no loop waits for another workgroup.  Inside k_hook every access to parent[] is an agent-scope relaxed
// atomic (the eight XCDs have L2s of their own: a plain load may return another XCD's stale line); k_flatten runs behind the
// kernel boundary and reads plainly.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_union_find.h"

namespace {

constexpr uint32_t kClusterThreads = 256;
constexpr uint64_t kEdgeCapDefault = 4096;   // borderline records the first hook pass has room for (RK_CLUSTER_EDGE_CAP)
constexpr double kBorderRel = 0x1p-46;       // the widening of rk_dist_rows: orders beyond the 2 ulps between the two logs

struct rk_edge {   // a borderline record: what rk_distance needs
    uint32_t row, col;
    int32_t common, size0, size1;
};

// counters of one call, 8 u32 words in front of the labels (one read-back brings both home)
enum { kCntHits = 0, kCntBorder = 1, kCntBad = 2, kCntWords = 4 };   // (u64 each)

__global__ void k_cluster_init(uint32_t *parent, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) parent[i] = i;
}

// n_hits_dev counts every hit of the join, those beyond `cap` included: the pass reads what was written.
__global__ void __launch_bounds__(kClusterThreads)
k_cluster_hook(const rk_hit *hits, const unsigned long long *n_hits_dev, unsigned long long cap, uint32_t *parent, uint32_t n,
               double link_below, rk_edge *edges, unsigned long long edge_cap, unsigned long long *n_border, unsigned long long *n_bad)
{
    const unsigned long long n_rec = min(*n_hits_dev, cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const rk_hit h = hits[e];
        if (h.row >= n || h.col >= n) {   // (never from the join's kernels; nothing is written through such an index)
            atomicAdd(n_bad, 1ULL);
            continue;
        }
        if (!(h.dist < link_below)) {
            const unsigned long long at = atomicAdd(n_border, 1ULL);
            if (at < edge_cap) edges[at] = rk_edge{h.row, h.col, h.common, h.size0, h.size1};
            continue;
        }
        uint32_t a = p_root(parent, h.row), b = p_root(parent, h.col);
        while (a != b) {
            const uint32_t hi = max(a, b), lo = min(a, b);
            uint32_t seen = hi;
            if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
            a = p_root(parent, seen);   // hi was linked meanwhile: seen < hi, on from there
            b = p_root(parent, lo);
        }
    }
}

// behind the kernel boundary: plain loads.  parent[] is not written here, so every thread walks a settled chain.
__global__ void k_cluster_flatten(const uint32_t *parent, uint32_t *label, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t x = i, p = parent[x];
        while (p != x) {
            x = p;
            p = parent[x];
        }
        label[i] = x;
    }
}

unsigned grid_for(const rk_ctx *ctx, uint64_t items)
{
    const uint64_t want = (items + kClusterThreads - 1) / kClusterThreads;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)std::max(1, ctx->num_cu) * 8));
}

// A dense report (-D above 1.0): every pair of a selected row and a later column is a hit, whatever it shares.  Rows are
// those of the index's internal order; the first selected row links everything behind it, the rows in front of it stay alone.
int cluster_dense(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, uint32_t *labels)
{
    const uint32_t N = idx->n_ref;
    const RowShard rows(o, N, N);
    const uint64_t first = (uint64_t)rows.row_first * rows.row_block;   // the first row of the first block of this shard
    std::iota(labels, labels + N, 0u);
    if (first + 1 >= N) return RK_OK;   // no selected row with a column behind it
    if (first == 0) {
        std::fill(labels, labels + N, 0u);
        return RK_OK;
    }
    std::vector<uint32_t> orig(N);
    int rc = rk_index_order(idx, orig.data());
    if (rc) return rc;
    uint32_t rep = 0xFFFFFFFFu;
    for (uint64_t i = first; i < N; i++) rep = std::min(rep, orig[i]);
    for (uint64_t i = first; i < N; i++) labels[orig[i]] = rep;
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_cluster_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t *labels_out, rk_cluster_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_cluster_stats st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    if (opts->triangle != 1) return rk_fail(ctx, RK_ERR_ARG, "rk_cluster_rows clusters a self join: triangle must be 1");
    const uint32_t N = idx->n_ref;
    if (!N) return RK_OK;
    if (!labels_out) return rk_fail(ctx, RK_ERR_ARG, "labels_out is null");
    if (int rc = rk_self_join_args(ctx, idx, opts)) return rc;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    if (rk_dense_mode(opts)) {
        if (!idx->d_selfrange && (idx->slices_refused || idx->H >= (1ULL << 30)))   // (what the join itself answers for a dense report over such an index)
            return rk_fail(ctx, RK_ERR_UNSUPPORTED, "this index has no slice records: only sparse self joins (a threshold below distance 1.0) run on it");
        int rc = cluster_dense(ctx, idx, opts, labels_out);
        if (rc) return rc;
        for (uint32_t i = 0; i < N; i++) st.n_clusters += labels_out[i] == i;
        if (stats) *stats = st;
        return RK_OK;
    }
    // The join reports with the widened threshold, the device links what lies below the narrowed one, the host decides the rest.
    // (-D within 2^-46 of 1.0 from below: the widening stops at 1.0 -- beyond it the public join would turn to the dense report.)
    rk_dist_opts widened = *opts;
    if (widened.max_dist > 0.0) widened.max_dist = std::min(widened.max_dist + widened.max_dist * kBorderRel, 1.0);
    const double link_below = opts->max_dist > 0.0 ? opts->max_dist - opts->max_dist * kBorderRel : opts->max_dist;
    hipStream_t stream = ctx->stream;

    uint64_t cap = rk_hit_capacity(RowShard(opts, N, N).n_rows());   // (the rows of this shard, as rk_dist_rows counts them)
    uint64_t edge_cap = kEdgeCapDefault;
    if (const char *e = getenv("RK_CLUSTER_EDGE_CAP")) edge_cap = std::max<uint64_t>(1, strtoull(e, nullptr, 10));

    DevBuf<uint32_t> parent(ctx), out(ctx);   // out: the counters (kCntWords u64), then the labels
    DevBuf<rk_edge> edges(ctx);
    RK_HIP(ctx, parent.alloc(N));
    RK_HIP(ctx, out.alloc((size_t)N + 2 * kCntWords));
    RK_HIP(ctx, edges.alloc(edge_cap));
    unsigned long long *cnt = (unsigned long long *)out.p;
    uint32_t *label = out.p + 2 * kCntWords;
    const size_t out_bytes = ((size_t)N + 2 * kCntWords) * 4;
    const unsigned char *home = nullptr;   // the context's page-locked scratch (asked for behind the join, whose lazy builders use it too)
    hipLaunchKernelGGL(k_cluster_init, dim3(grid_for(ctx, N)), dim3(kClusterThreads), 0, stream, parent.p, N);
    RK_HIP(ctx, hipGetLastError());
    if (ctx->timing) ctx->last_ms[RK_MS_CLUSTER_HOOK] = 0.0;

    unsigned long long n_hits = 0, n_border = 0;
    bool done = false;
    for (int attempt = 0; attempt < 2 && !done; attempt++) {
        DevBuf<rk_hit> hits(ctx);
        if (hits.alloc(cap) != hipSuccess) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu hit records on the device", (unsigned long long)cap);
        RK_HIP(ctx, hipMemsetAsync(cnt, 0, kCntWords * 8, stream));
        int rc = rk_dist_rows_dev(ctx, idx, nullptr, &widened, hits.p, cap, (uint64_t *)(cnt + kCntHits), stream);
        if (rc) return rc;
        st.join_attempts++;
        st.hook_attempts = 0;
        for (int pass = 0; pass < 2 && !done; pass++) {
            if (ctx->timing) RK_HIP(ctx, hipEventRecord(ctx->ev[0], stream));
            hipLaunchKernelGGL(k_cluster_hook, dim3(grid_for(ctx, cap)), dim3(kClusterThreads), 0, stream, hits.p, cnt + kCntHits, (unsigned long long)cap,
                               parent.p, N, link_below, edges.p, (unsigned long long)edge_cap, cnt + kCntBorder, cnt + kCntBad);
            if (ctx->timing) RK_HIP(ctx, hipEventRecord(ctx->ev[1], stream));
            RK_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_cluster_flatten, dim3(grid_for(ctx, N)), dim3(kClusterThreads), 0, stream, parent.p, label, N);
            RK_HIP(ctx, hipGetLastError());
            home = (const unsigned char *)rk_pinned_scratch(ctx, out_bytes);
            if (!home) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %zu bytes of page-locked memory for the labels", out_bytes);
            RK_HIP(ctx, hipMemcpyAsync((void *)home, out.p, out_bytes, hipMemcpyDeviceToHost, stream));
            RK_HIP(ctx, hipStreamSynchronize(stream));
            unsigned long long c[kCntWords];
            memcpy(c, home, sizeof c);
            if (c[kCntBad]) return rk_fail(ctx, RK_ERR_HIP, "%llu hit records name a genome beyond the index", c[kCntBad]);
            n_hits = c[kCntHits];
            n_border = c[kCntBorder];
            if (n_hits > cap) {   // overflow: the join again with the exact count (the links made so far are links of the result)
                cap = n_hits;
                break;
            }
            st.hook_attempts++;
            if (ctx->timing) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->last_ms[RK_MS_CLUSTER_HOOK] = ms;
            }
            if (n_border > edge_cap) {   // the hook pass alone again, with room for every borderline record (linking twice changes nothing)
                edge_cap = n_border;
                RK_HIP(ctx, edges.alloc(edge_cap));
                RK_HIP(ctx, hipMemsetAsync(cnt + kCntBorder, 0, 8, stream));
                continue;
            }
            done = true;
        }
        if (done && n_border) {   // before `hits` and `edges` go back to the pool
            std::vector<rk_edge> e(n_border);
            RK_HIP(ctx, hipMemcpyAsync(e.data(), edges.p, n_border * sizeof(rk_edge), hipMemcpyDeviceToHost, stream));
            RK_HIP(ctx, hipStreamSynchronize(stream));
            std::vector<rk_hit> h(n_border);
            for (size_t i = 0; i < e.size(); i++) h[i] = rk_hit{e[i].row, e[i].col, e[i].common, e[i].size0, e[i].size1, 0, 0.0, 0.0};
            st.borderline_kept = rk_host_exact_distances(h.data(), n_border, opts);
            h.resize(st.borderline_kept);
            memcpy(labels_out, home + kCntWords * 8, (size_t)N * 4);
            for (const rk_hit &k : h) host_union(labels_out, k.row, k.col);
        } else if (done) {
            memcpy(labels_out, home + kCntWords * 8, (size_t)N * 4);
        }
    }
    if (!done) return rk_fail(ctx, RK_ERR_CAPACITY, "hit or borderline buffer overflow persisted after resize");
    st.edges = n_hits;
    st.borderline = n_border;
    st.n_clusters = host_flatten(labels_out, N);
    if (stats) *stats = st;
    return RK_OK;
}

int rk_cluster_merge(const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out)
{
    if (!a || !b || !out) return RK_ERR_ARG;
    for (uint32_t i = 0; i < n; i++)
        if (a[i] >= n || b[i] >= n) return RK_ERR_ARG;
    // both arrays as edge lists (i, label): right for any entries below n, not only for canonical labels
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    for (uint32_t i = 0; i < n; i++) {
        host_union(parent.data(), i, a[i]);
        host_union(parent.data(), i, b[i]);
    }
    host_flatten(parent.data(), n);
    if (n) memcpy(out, parent.data(), (size_t)n * 4);
    return RK_OK;
}

}  // extern "C"
