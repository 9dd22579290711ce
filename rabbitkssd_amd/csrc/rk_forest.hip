// rk_forest.hip -- the minimum spanning forest of `alldist` on the device (rk_forest_rows) and its host side: the fold of two
// forests (rk_forest_merge) and the cut at a threshold (rk_forest_cut).  The forest of the "reportable pair" graph is the
// single-linkage dendrogram up to -D: cut at any t <= D it gives the clusters rk_cluster_rows returns at t, without a join.
//
// Order of edges (include/rabbitkssd.h, clusters section): the ratio common / u descending -- u = size0 + size1 - common (metric 0)
// or min(size0, size1) (metric 1); both distances fall strictly as it rises --, then row ascending, then col ascending.  Strict,
// so the forest is unique: the edges Kruskal accepts in this order.  On the device the ratio is the 64-bit key
// floor(common * 2^62 / u), exact for 0 < common <= u < 2^31 (distinct fractions differ by more than 2^-62); `w` = ~key turns
// "nearest first" into an unsigned minimum.
//
//   stage     rk_edge_stage.h: the self join into a device buffer, its key pass (EdgeStage::key_pass<false>: per record w and
//             row << 32 | col; a BORDERLINE record and a record outside 0 < common <= u -- multisets: no key -- go to the small host
//             buffer and are dead on the device), the two retries, the host's decision about the records of that buffer;
//   rounds    Boruvka (rk_boruvka.h, shared with rk_mreach.hip): k_match_w (atomic minimum of w per component, both endpoints),
//             k_match_rc (among the records that match that w, atomic minimum of row << 32 | col), k_link (a record that is the best
//             edge of either of its components is appended once to the forest buffer, its roots linked with the compare-and-swap
//             hook), k_flatten (label[i] = root(i), best arrays reset).  The host reads one counter per round and stops when a round
//             appended nothing;
//   sort      the <= N - 1 forest records by (w, row, col): two stable radix passes; download;
//   host      Kruskal over (forest + the records the stage kept), jorc / dist of the result recomputed with the C library's log.
//
// Termination and acyclicity: DESIGN.md 4.7.  In short: the order is strict, so the best edges of one round form a forest over the
// round's components (a cycle would need an edge that is smaller than itself), apart from the edge both of its components chose,
// which is ONE record and whose single thread appends it once.  Hence every k_link thread unites two different trees, whatever
// the others do meanwhile, and its compare-and-swap loop ends as k_cluster_hook's does.  No loop waits for another workgroup.
// Memory scope: label[] and the best arrays are written by one kernel and read by the next (plain loads behind the kernel
// boundary; the minima themselves are agent-scope atomics); parent[] inside k_link only through agent-scope relaxed atomics.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_union_find.h"
#include "rk_edge_order.h"
#include "rk_edge_stage.h"
#include "rk_boruvka.h"

namespace {

// sort keys of the forest records: pass 0 row << 32 | col, pass 1 w (the radix sort is stable)
__global__ void k_forest_sort_keys(const rk_hit *forest, unsigned long long n, int metric, int pass, unsigned long long *keys)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rk_hit h = forest[i];
    if (!pass) {
        keys[i] = ((unsigned long long)h.row << 32) | h.col;
        return;
    }
    long long c, u;
    ratio_terms(h.common, h.size0, h.size1, metric, &c, &u);
    keys[i] = ~ratio_key((unsigned long long)c, (unsigned long long)u);   // (only records k_edge_keys gave a key are here)
}

bool edges_within(const rk_hit *e, uint64_t m, uint32_t n)
{
    for (uint64_t i = 0; i < m; i++)
        if (e[i].row >= n || e[i].col >= n) return false;
    return true;
}

}  // namespace

extern "C" {

int rk_forest_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, rk_hit **edges_out, uint64_t *n_edges, rk_forest_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_forest_stats st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    if (!edges_out || !n_edges) return rk_fail(ctx, RK_ERR_ARG, "edges_out or n_edges is null");
    *edges_out = nullptr;
    *n_edges = 0;
    const StageNeeds needs{"rk_forest_rows", nullptr, true};
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    const uint32_t N = idx->n_ref;
    if (!N) return RK_OK;
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassKeys);
    const int metric = stage.metric;
    const uint64_t forest_cap = N - 1;
    uint32_t max_rounds = 2;   // 2 + ceil(log2 N): the components with an edge left at least halve per round, the last round appends nothing
    while ((1ULL << (max_rounds - 2)) < N) max_rounds++;

    DevBuf<uint32_t> parent(ctx), label(ctx);
    DevBuf<unsigned long long> best_w(ctx), best_rc(ctx), n_forest_dev(ctx), w(ctx), rc_(ctx);
    DevBuf<rk_hit> forest(ctx);
    RK_HIP(ctx, parent.alloc(N));
    RK_HIP(ctx, label.alloc(N));
    RK_HIP(ctx, best_w.alloc(N));
    RK_HIP(ctx, best_rc.alloc(N));
    RK_HIP(ctx, n_forest_dev.alloc(1));
    RK_HIP(ctx, forest.alloc(forest_cap));
    RK_HIP(ctx, hipMemsetAsync(n_forest_dev.p, 0, 8, stream));
    hipLaunchKernelGGL(k_forest_init, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, parent.p, label.p, best_w.p, best_rc.p, N);
    RK_HIP(ctx, hipGetLastError());

    // the key pass: nothing is linked before the stage is through
    int rc = stage.run([&](int pass) { return stage.key_pass<false>(pass, w, rc_); });
    if (rc) return rc;
    stage.stats(&st);
    const rk_hit *hits = stage.hits.p;
    const unsigned long long *n_hits_dev = stage.cnt() + kCntHits, cap = stage.cap;
    const unsigned grid = grid_for(ctx, cap);
    // Boruvka rounds; the host reads one counter per round
    unsigned long long n_forest = 0;
    bool settled = stage.n_hits == stage.n_border;   // no record takes part: no round
    while (!settled) {
        if (st.rounds == max_rounds) return rk_fail(ctx, RK_ERR_HIP, "rk_forest_rows: %u rounds did not settle the forest of %u genomes (internal error)", max_rounds, N);
        hipLaunchKernelGGL(k_forest_match_w, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_hits_dev, cap, label.p, best_w.p);
        hipLaunchKernelGGL(k_forest_match_rc, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_hits_dev, cap, label.p, best_w.p, best_rc.p);
        hipLaunchKernelGGL(k_forest_link, dim3(grid), dim3(kStageThreads), 0, stream, hits, w.p, rc_.p, n_hits_dev, cap, label.p, best_w.p, best_rc.p, parent.p,
                           forest.p, (unsigned long long)forest_cap, n_forest_dev.p);
        hipLaunchKernelGGL(k_forest_flatten, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, parent.p, label.p, best_w.p, best_rc.p, N);
        RK_HIP(ctx, hipGetLastError());
        unsigned long long now = 0;
        if (int r = rk_read_back(ctx, &now, n_forest_dev.p, 8, stream)) return r;
        st.rounds++;
        if (now > forest_cap) return rk_fail(ctx, RK_ERR_HIP, "rk_forest_rows: %llu forest records for %u genomes (internal error)", now, N);
        settled = now == n_forest;
        n_forest = now;
    }
    // the forest in order: by (row, col), then stably by w
    std::vector<rk_hit> all(n_forest);   // the forest of the device, then the kept borderline records
    if (n_forest) {
        DevBuf<rk_hit> tmp(ctx);
        DevBuf<unsigned long long> keys(ctx), keys_out(ctx);
        if (tmp.alloc(n_forest) != hipSuccess || keys.alloc(n_forest) != hipSuccess || keys_out.alloc(n_forest) != hipSuccess)
            return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate the sort buffers of %llu forest records", n_forest);
        const unsigned sgrid = (unsigned)((n_forest + kStageThreads - 1) / kStageThreads);
        hipLaunchKernelGGL(k_forest_sort_keys, dim3(sgrid), dim3(kStageThreads), 0, stream, forest.p, n_forest, metric, 0, keys.p);
        RK_HIP(ctx, hipGetLastError());
        if (int r = rk_prim_sort_hits(ctx, keys.p, keys_out.p, forest.p, tmp.p, n_forest, 64, stream)) return rk_fail(ctx, r, "sorting the forest records failed");
        hipLaunchKernelGGL(k_forest_sort_keys, dim3(sgrid), dim3(kStageThreads), 0, stream, tmp.p, n_forest, metric, 1, keys.p);
        RK_HIP(ctx, hipGetLastError());
        if (int r = rk_prim_sort_hits(ctx, keys.p, keys_out.p, tmp.p, forest.p, n_forest, 64, stream)) return rk_fail(ctx, r, "sorting the forest records failed");
        RK_HIP(ctx, hipMemcpyAsync(all.data(), forest.p, n_forest * sizeof(rk_hit), hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipStreamSynchronize(stream));
    }
    std::vector<rk_hit> h;
    if ((rc = stage.decide(&h))) return rc;
    st.borderline_kept = h.size();
    if (!h.empty()) {
        std::sort(h.begin(), h.end(), EdgeLess{metric});
        const size_t mid = all.size();
        all.insert(all.end(), h.begin(), h.end());
        std::inplace_merge(all.begin(), all.begin() + mid, all.end(), EdgeLess{metric});
    }
    // MSF(E1 + E2) = MSF(MSF(E1) + E2): Kruskal over the device's forest and the kept records.  (Without kept records it accepts
    // every edge -- the device's forest is one.)
    const uint64_t device_edges = all.size() - st.borderline_kept;
    const uint64_t kept = kruskal_sorted(all.data(), all.size(), N);
    if (!st.borderline_kept && kept != device_edges) return rk_fail(ctx, RK_ERR_HIP, "rk_forest_rows: the device's forest holds a cycle (internal error)");
    // the reference's values bit for bit (a record the device linked lies below the exact threshold: none is dropped)
    if (rk_host_exact_distances(all.data(), kept, opts) != kept) return rk_fail(ctx, RK_ERR_HIP, "rk_forest_rows: a linked record lies beyond the exact threshold (internal error)");
    rk_hit *out = host_records(kept);
    if (!out) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu forest records failed", (unsigned long long)kept);
    if (kept) memcpy(out, all.data(), kept * sizeof(rk_hit));
    *edges_out = out;
    *n_edges = kept;
    st.n_trees = N - (uint32_t)kept;
    if (stats) *stats = st;
    return RK_OK;
}

int rk_forest_merge(const rk_hit *a, uint64_t na, const rk_hit *b, uint64_t nb, uint32_t n, int metric, rk_hit **out, uint64_t *n_out)
{
    if (!out || !n_out || (na && !a) || (nb && !b)) return RK_ERR_ARG;
    if (!edges_within(a, na, n) || !edges_within(b, nb, n)) return RK_ERR_ARG;
    rk_hit *all = host_records(na + nb);
    if (!all) return RK_ERR_NOMEM;
    if (na) memcpy(all, a, na * sizeof(rk_hit));
    if (nb) memcpy(all + na, b, nb * sizeof(rk_hit));
    std::sort(all, all + na + nb, EdgeLess{metric != 0});
    *n_out = kruskal_sorted(all, na + nb, n);
    *out = all;
    return RK_OK;
}

int rk_forest_cut(const rk_hit *edges, uint64_t n_edges, uint32_t n, double max_dist, uint32_t *labels_out)
{
    if ((n_edges && !edges) || (n && !labels_out)) return RK_ERR_ARG;
    if (!edges_within(edges, n_edges, n)) return RK_ERR_ARG;
    std::iota(labels_out, labels_out + n, 0u);
    for (uint64_t i = 0; i < n_edges; i++)
        if (edges[i].dist < max_dist) host_union(labels_out, edges[i].row, edges[i].col);
    host_flatten(labels_out, n);
    return RK_OK;
}

}  // extern "C"
