// rk_cluster.hip -- single-linkage clusters of `alldist` on the device (rk_cluster_rows) and the host fold of two label
// arrays (rk_cluster_merge).  The users of `alldist -D d` feed its hit list into a union-find; here the components of the
// "reportable pair" graph are computed where the hit records already are: nothing of size O(hits) crosses PCIe, nothing is
// sorted, no host libm pass over the hits.
//
//   stage    rk_edge_stage.h: the self join into a device buffer, the first pass below, its two retries, the borderline records
//            decided on the host.  The labels are the tail of its counter block: one read-back brings counters and labels home;
//   k_init   parent[i] = i, indexed by the CALLER's genome index (rk_hit.row / .col carry caller indices);
//   k_hook   the first pass, one grid-stride sweep over the records: a record whose device distance is below D (1 - 2^-46) links
//            the roots of its two genomes, larger under smaller, with a compare-and-swap on the larger root (p_link); every other
//            record is BORDERLINE: appended to the stage's buffer for the host, not linked.  parent[] is not reset between the
//            stage's attempts: a link made once is a link of the result, and linking twice changes nothing;
//   k_flatten  label[i] = root(i) = the smallest caller index of i's component;
//   host     the records the stage kept are united into the labels.
//
// Termination and memory scope of k_hook: DESIGN.md 4.6.  In short: parent[x] <= x at every moment and a root is only ever
// linked under a smaller index, so every chain strictly decreases and every failed compare-and-swap has observed a strictly
// smaller parent -- no loop waits for another workgroup.  Inside k_hook every access to parent[] is an agent-scope relaxed
// atomic (the eight XCDs have L2s of their own: a plain load may return another XCD's stale line); k_flatten runs behind the
// kernel boundary and reads plainly.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_union_find.h"
#include "rk_edge_stage.h"

namespace {

__global__ void k_cluster_init(uint32_t *parent, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) parent[i] = i;
}

// cnt[kCntHits] counts every hit of the join, those beyond `cap` included: the pass reads what was written.
__global__ void __launch_bounds__(kStageThreads)
k_cluster_hook(const rk_hit *hits, unsigned long long *cnt, unsigned long long cap, uint32_t *parent, uint32_t n, double link_below, rk_edge *edges,
               unsigned long long edge_cap)
{
    const unsigned long long n_rec = min(cnt[kCntHits], cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const rk_hit h = hits[e];
        if (h.row >= n || h.col >= n) {   // (never from the join's kernels; nothing is written through such an index)
            atomicAdd(cnt + kCntBad, 1ULL);
            continue;
        }
        if (!(h.dist < link_below)) {
            edge_append(h, e, edges, nullptr, edge_cap, cnt + kCntBorder);
            continue;
        }
        p_link(parent, h.row, h.col);
    }
}

__global__ void k_cluster_flatten(const uint32_t *parent, uint32_t *label, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) label[i] = p_settled_root(parent, i);
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
    const StageNeeds needs{"rk_cluster_rows", nullptr, false};   // (every shard, and the dense report answered below)
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    const uint32_t N = idx->n_ref;
    if (!N) return RK_OK;
    if (!labels_out) return rk_fail(ctx, RK_ERR_ARG, "labels_out is null");
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
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
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassOwn, (size_t)N * 4);   // the tail: the labels
    const TimedSpan span{ctx, RK_MS_CLUSTER_HOOK};
    DevBuf<uint32_t> parent(ctx);
    RK_HIP(ctx, parent.alloc(N));
    hipLaunchKernelGGL(k_cluster_init, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, parent.p, N);
    RK_HIP(ctx, hipGetLastError());
    span.clear();
    int rc = stage.run([&](int) -> int {
        RK_HIP(ctx, span.begin());
        hipLaunchKernelGGL(k_cluster_hook, dim3(grid_for(ctx, stage.cap)), dim3(kStageThreads), 0, stream, stage.hits.p, stage.cnt(),
                           (unsigned long long)stage.cap, parent.p, N, stage.link_below, stage.edges.p, (unsigned long long)stage.edge_cap);
        RK_HIP(ctx, span.end());
        RK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_cluster_flatten, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, parent.p, (uint32_t *)stage.tail(), N);
        RK_HIP(ctx, hipGetLastError());
        return RK_OK;
    });
    if (rc) return rc;
    span.read();   // (the events of the last pass)
    std::vector<rk_hit> kept;
    if ((rc = stage.decide(&kept))) return rc;
    memcpy(labels_out, stage.home_tail(), (size_t)N * 4);
    for (const rk_hit &k : kept) host_union(labels_out, k.row, k.col);
    st.join_attempts = stage.join_attempts;
    st.hook_attempts = stage.pass_attempts;
    st.edges = stage.n_hits;
    st.borderline = stage.n_border;
    st.borderline_kept = kept.size();
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
