// rk_mreach.hip -- the minimum spanning forest of `alldist` under MUTUAL-REACHABILITY distance, the HDBSCAN* hierarchy up to -D, on the
// device (rk_mreach_rows), the same rule on the host over a hit list the caller already has (rk_mreach_hits) and the cut of the forest
// at a threshold (rk_mreach_cut).  The graph is that of rk_cluster_rows.  With k = min_pts - 1 the CORE RECORD of genome v is the k-th
// record of v's list in the order of rk_knn_rows (ratio descending, exactly, then the neighbour's caller index); the weight of record
// e = (a, b) is mw(e) = max(w(e), core_w[a], core_w[b]) with w = ~ratio key and core_w[v] the w of v's core record -- 0 for k = 0,
// infinite (kDead) for a genome with fewer than k records, which no edge touches --; the forest is what Kruskal accepts in the order
// (mw, row, col).  include/rabbitkssd.h, mutual-reachability forest.
//
//   stage     rk_edge_stage.h: the self join into a device buffer, its key pass (EdgeStage::key_pass<true>: per record w and
//             row << 32 | col; a BORDERLINE record goes, with its slot number, to the small host buffer and is dead for now; a record
//             outside 0 < common <= u -- multisets -- is counted: the call refuses such a collection), the two retries;
//   host      the stage decides the borderline records BEFORE anything else (one kept edge changes a core distance, and with it the
//             weight of edges arbitrarily far away: no fold afterwards is possible); the slot numbers of the kept ones go back up and
//             k_edge_revive gives them their keys;
//   core      (k >= 1) k_edge_degree, the scan of the degrees, k_knn_fill and one wave64 per genome running the selection of
//             rk_knn_select.h (k_mreach_core): lane k - 1 ends up with the k-th entry and writes core_w[v] and core_e[v], the record's
//             number -- (kDead, RK_MREACH_NONE) where deg(v) < k;
//   weights   k_mreach_weights, one sweep: a live record gets w = max(w, core_w[row], core_w[col]); kDead is the largest value, so a
//             record at a genome without a core record dies by the same maximum;
//   rounds    rk_boruvka.h over w and row << 32 | col, k_forest_link storing the winning w beside each appended record (mw is not a
//             function of the record alone);
//   sort      the <= N - 1 forest records by (mw, row, col): the stored mw travels in the record's dist field (the host recomputes
//             that field anyway), two stable radix passes; k_mreach_gather collects hits[core_e[v]] into N records;
//   host      both buffers come home (40 (N - 1) + 40 N bytes at most, never O(hits)); jorc / dist recomputed with the C library's
//             log; a Kruskal that must accept every edge; core_dist_out and core_nb_out.
//
// Memory scope: w[], rc[], deg[], aoff[], cur[], the entries, core_w[] and core_e[] are written by one kernel and read by a later one
// on the same stream (plain accesses behind kernel boundaries); inside a kernel only the relaxed agent-scope atomics of the degree,
// the fill and rk_boruvka.h.  k_mreach_core has no barrier: the waves of a workgroup have different trip counts.  Termination: the
// argument of rk_boruvka.h -- it asks of w only that (w, row, col) is a strict order, and a pair has one record; that most records tie
// in w here (every edge inside a dense clade carries a core distance) costs nothing but work for the second minimum.  DESIGN.md 4.11.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_edge_order.h"
#include "rk_union_find.h"
#include "rk_edge_stage.h"
#include "rk_knn_select.h"
#include "rk_boruvka.h"

namespace {

constexpr uint32_t kNone = RK_MREACH_NONE;

// 1 <= k <= 64: the selection of rk_knn_select.h; lane k - 1 holds the k-th entry of v's list, or (kDead, kDead) where deg(v) < k
__global__ void __launch_bounds__(kStageThreads)
k_mreach_core(const KnnEntry *adj, const uint32_t *aoff, uint32_t n, uint32_t k, unsigned long long *core_w, uint32_t *core_e)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t n_waves = (gridDim.x * blockDim.x) / kWave;
    for (uint32_t v = (blockIdx.x * blockDim.x + threadIdx.x) / kWave; v < n; v += n_waves) {
        const unsigned long long beg = aoff[v], end = aoff[v + 1];
        unsigned long long bw, bx;
        knn_select_wave(adj, beg, end, lane, k, &bw, &bx);
        if (lane == k - 1) {
            const bool has = end - beg >= k;
            core_w[v] = has ? bw : kDead;
            core_e[v] = has ? (uint32_t)bx : kNone;
        }
    }
}

// core_w[] is final: written by k_mreach_core, a kernel boundary away
__global__ void __launch_bounds__(kStageThreads)
k_mreach_weights(unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const unsigned long long *core_w)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        w[e] = max(we, max(core_w[(uint32_t)(p >> 32)], core_w[(uint32_t)p]));   // (kDead: an endpoint without a core record)
    }
}

// sort keys of the forest records: pass 0 row << 32 | col -- and the record's mw moves into its dist field, to travel with it --,
// pass 1 that mw (the radix sort is stable)
__global__ void k_mreach_sort_keys(rk_hit *forest, const unsigned long long *forest_w, unsigned long long n, int pass, unsigned long long *keys)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!pass) {
        const unsigned long long mw = forest_w[i];
        memcpy(&forest[i].dist, &mw, 8);
        keys[i] = ((unsigned long long)forest[i].row << 32) | forest[i].col;
        return;
    }
    unsigned long long mw;
    memcpy(&mw, &forest[i].dist, 8);
    keys[i] = mw;
}

// out[v] = the core record of v, or a record of no genome (core_e[v] is a record number k_knn_fill wrote: below n_rec)
__global__ void k_mreach_gather(const rk_hit *hits, const uint32_t *core_e, unsigned long long n_rec, uint32_t n, rk_hit *out)
{
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        const uint32_t e = core_e[v];
        out[v] = e < n_rec ? hits[e] : rk_hit{kNone, kNone, 0, 0, 0, 0, 0.0, 0.0};
    }
}

// ---- host: the rule over a hit list -----------------------------------------------------------------------------------------
// the weight of a record in exact terms: its ratio, smaller ratio = heavier; a record without a ratio is heavier than every record
// that has one (EdgeLess puts it behind them)
struct Ratio {
    long long c, u;
    bool valid;
};

inline Ratio ratio_of(const rk_hit &h, int metric)
{
    Ratio r;
    ratio_terms(h.common, h.size0, h.size1, metric, &r.c, &r.u);
    r.valid = r.u > 0 && r.c >= 0;
    return r;
}

inline bool lighter(const Ratio &a, const Ratio &b)
{
    if (a.valid != b.valid) return a.valid;
    return a.valid && (__int128)a.c * b.u > (__int128)b.c * a.u;
}

inline Ratio heavier_of(const Ratio &a, const Ratio &b) { return lighter(a, b) ? b : a; }

struct Result {
    std::vector<int64_t> core;   // per genome the number of its core record in the hit list, -1: none
    std::vector<rk_hit> edges;   // the forest, in order
    uint32_t n_core = 0;         // genomes with a finite core distance
};

// (hits validated by the caller; min_pts >= 1)
void mreach_of_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t min_pts, int metric, Result *r)
{
    const uint64_t k = min_pts - 1;
    r->core.assign(n, -1);
    r->edges.clear();
    r->n_core = k ? 0 : n;
    if (k) {
        std::vector<uint64_t> start, adj;
        hit_adjacency(hits, n_hits, n, &start, &adj);
        for (uint32_t v = 0; v < n; v++) {
            if (start[v + 1] - start[v] < k) continue;
            uint64_t *first = adj.data() + start[v], *last = adj.data() + start[v + 1], *kth = first + (k - 1);
            const NeighbourLess nearer{metric, v};
            std::nth_element(first, kth, last, [&](uint64_t a, uint64_t b) { return nearer(hits[a], hits[b]); });
            r->core[v] = (int64_t)*kth;
            r->n_core++;
        }
    }
    // the records with a finite weight, their mw, the order (mw, smaller endpoint, larger endpoint)
    std::vector<uint64_t> order;
    std::vector<Ratio> mw(n_hits);
    for (uint64_t e = 0; e < n_hits; e++) {
        mw[e] = ratio_of(hits[e], metric);
        if (k) {
            const int64_t ca = r->core[hits[e].row], cb = r->core[hits[e].col];
            if (ca < 0 || cb < 0) continue;
            mw[e] = heavier_of(mw[e], heavier_of(ratio_of(hits[ca], metric), ratio_of(hits[cb], metric)));
        }
        order.push_back(e);
    }
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (lighter(mw[a], mw[b])) return true;
        if (lighter(mw[b], mw[a])) return false;
        const uint32_t a0 = std::min(hits[a].row, hits[a].col), a1 = std::max(hits[a].row, hits[a].col);
        const uint32_t b0 = std::min(hits[b].row, hits[b].col), b1 = std::max(hits[b].row, hits[b].col);
        return a0 != b0 ? a0 < b0 : a1 < b1;
    });
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    for (uint64_t e : order)
        if (host_union(parent.data(), hits[e].row, hits[e].col)) r->edges.push_back(hits[e]);
}

// core_dist / core_nb of a result whose core records are hits[core[v]]
void hand_over_cores(const Result &r, const rk_hit *hits, uint32_t n, uint32_t min_pts, double *core_dist_out, uint32_t *core_nb_out)
{
    for (uint32_t v = 0; v < n; v++) {
        const bool has = r.core[v] >= 0;
        core_dist_out[v] = min_pts == 1 ? 0.0 : has ? hits[r.core[v]].dist : std::numeric_limits<double>::infinity();
        if (core_nb_out) core_nb_out[v] = has ? other_end(hits[r.core[v]], v) : kNone;
    }
}

int hand_over_edges(const std::vector<rk_hit> &rec, rk_hit **out, uint64_t *n_out)
{
    rk_hit *p = host_records(rec.size());
    if (!p) return RK_ERR_NOMEM;
    if (!rec.empty()) memcpy(p, rec.data(), rec.size() * sizeof(rk_hit));
    *out = p;
    *n_out = rec.size();
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_mreach_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t min_pts, int metric, double *core_dist_out, uint32_t *core_nb_out,
                   rk_hit **edges_out, uint64_t *n_edges)
{
    if ((n_hits && !hits) || (n && !core_dist_out) || !edges_out || !n_edges || !min_pts) return RK_ERR_ARG;
    for (uint64_t e = 0; e < n_hits; e++)
        if (hits[e].row >= n || hits[e].col >= n || hits[e].row == hits[e].col) return RK_ERR_ARG;
    Result r;
    mreach_of_hits(hits, n_hits, n, min_pts, metric != 0, &r);
    if (int rc = hand_over_edges(r.edges, edges_out, n_edges)) return rc;
    hand_over_cores(r, hits, n, min_pts, core_dist_out, core_nb_out);
    return RK_OK;
}

int rk_mreach_cut(const rk_hit *edges, uint64_t n_edges, const double *core_dist, uint32_t n, double t, uint32_t *labels_out)
{
    if ((n_edges && !edges) || (n && (!core_dist || !labels_out))) return RK_ERR_ARG;
    for (uint64_t i = 0; i < n_edges; i++)
        if (edges[i].row >= n || edges[i].col >= n) return RK_ERR_ARG;
    std::iota(labels_out, labels_out + n, 0u);
    for (uint64_t i = 0; i < n_edges; i++)
        if (std::max(edges[i].dist, std::max(core_dist[edges[i].row], core_dist[edges[i].col])) < t) host_union(labels_out, edges[i].row, edges[i].col);
    host_flatten(labels_out, n);
    for (uint32_t v = 0; v < n; v++)   // (a root is the smallest index of its component, and only core genomes are linked)
        if (!(core_dist[v] < t)) labels_out[v] = RK_DBSCAN_NOISE;
    return RK_OK;
}

int rk_mreach_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t min_pts, double *core_dist_out, uint32_t *core_nb_out,
                   rk_hit **edges_out, uint64_t *n_edges, rk_mreach_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_mreach_stats st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    if (!edges_out || !n_edges) return rk_fail(ctx, RK_ERR_ARG, "edges_out or n_edges is null");
    *edges_out = nullptr;
    *n_edges = 0;
    const uint32_t N = idx->n_ref;
    if (N && !core_dist_out) return rk_fail(ctx, RK_ERR_ARG, "core_dist_out is null");
    if (!min_pts) return rk_fail(ctx, RK_ERR_ARG, "rk_mreach_rows: min_pts counts the genome itself and must be 1 or more");
    const StageNeeds needs{"rk_mreach_rows", "the core distances of a row shard are partial, and the weights do not compose from shards", true};
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    if (!N) return RK_OK;
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
    const TimedSpan span{ctx, RK_MS_MREACH};
    span.clear();
    const int metric = opts->metric != 0;
    const uint32_t k = min_pts - 1;
    const double inf = std::numeric_limits<double>::infinity();

    // the same rule over the hit list on the host: what the device path has no room for, and the A/B leg of tools/mreach_probe.py
    auto on_the_host = [&]() -> int {
        rk_hit *hits = nullptr;
        uint64_t n_hits = 0;
        if (int rc = rk_dist_rows(ctx, idx, nullptr, opts, &hits, &n_hits, nullptr)) return rc;
        unsigned long long out_of_range = 0;
        for (uint64_t e = 0; e < n_hits; e++) {
            const Ratio q = ratio_of(hits[e], metric);
            out_of_range += !(q.c > 0 && q.c <= q.u);
        }
        if (out_of_range) {
            rk_free_host(hits);
            return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: %llu hit records lie outside 0 < common <= u (sketches that repeat hashes): they have no place in the order",
                           needs.who, out_of_range);
        }
        Result r;
        mreach_of_hits(hits, n_hits, N, min_pts, metric, &r);
        hand_over_cores(r, hits, N, min_pts, core_dist_out, core_nb_out);
        rk_free_host(hits);
        if (hand_over_edges(r.edges, edges_out, n_edges)) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu forest records failed", (unsigned long long)r.edges.size());
        memset(&st, 0, sizeof st);
        st.edges = n_hits;
        st.n_trees = N - (uint32_t)r.edges.size();
        st.n_core = r.n_core;
        st.path = 2;
        if (stats) *stats = st;
        return RK_OK;
    };
    if (k > kKnnDeviceMax || rk_switched_off("RK_MREACH_DEVICE")) return on_the_host();

    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassGreedyKeys);   // with slot numbers
    DevBuf<unsigned long long> w(ctx), rc_(ctx);
    int rc = stage.run([&](int pass) { return stage.key_pass<true>(pass, w, rc_); });
    if (stage.beyond_31_bits(rc)) {   // the entries number the records in 31 bits
        w.reset();
        rc_.reset();
        return on_the_host();
    }
    if (rc) return rc;
    stage.stats(&st);
    st.path = 1;
    // the borderline records, decided before anything else
    if ((rc = stage.revive(w.p, &st.borderline_kept))) return rc;
    const unsigned long long n_rec = stage.n_hits;
    const unsigned grid = grid_for(ctx, n_rec), vgrid = grid_for(ctx, (uint64_t)N + 1);
    const unsigned long long n_live = n_rec - stage.n_border + st.borderline_kept;

    std::vector<rk_hit> forest_h, core_h;   // the forest in order; per genome its core record (k >= 1)
    if (n_live) {
        RK_HIP(ctx, span.begin());
        DevBuf<uint32_t> core_e(ctx);
        // core records
        if (k) {
            DevBuf<uint32_t> deg(ctx), kmin(ctx), aoff(ctx), most(ctx);
            DevBuf<unsigned long long> core_w(ctx);
            DevBuf<KnnEntry> adj(ctx);
            RK_HIP(ctx, deg.alloc((size_t)N + 1));
            RK_HIP(ctx, kmin.alloc((size_t)N + 1));
            RK_HIP(ctx, aoff.alloc((size_t)N + 1));
            RK_HIP(ctx, most.alloc(1));
            RK_HIP(ctx, core_w.alloc(N));
            RK_HIP(ctx, core_e.alloc(N));
            if (adj.alloc(2 * n_live) != hipSuccess) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate the adjacency of %llu hit records on the device", n_live);
            RK_HIP(ctx, hipMemsetAsync(deg.p, 0, ((size_t)N + 1) * 4, stream));
            RK_HIP(ctx, hipMemsetAsync(most.p, 0, 4, stream));
            hipLaunchKernelGGL(k_edge_degree, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, deg.p);
            hipLaunchKernelGGL(k_knn_offsets, dim3(vgrid), dim3(kStageThreads), 0, stream, deg.p, kmin.p, N, k, most.p);
            RK_HIP(ctx, hipGetLastError());
            if (int r = rk_prim_exclusive_scan_u32(ctx, deg.p, aoff.p, (uint64_t)N + 1, stream)) return rk_fail(ctx, r, "rk_mreach_rows: the scan of the degrees failed");
            RK_HIP(ctx, hipMemsetAsync(deg.p, 0, (size_t)N * 4, stream));   // from here on the cursors of the fill
            hipLaunchKernelGGL(k_knn_fill, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, aoff.p, deg.p, adj.p);
            const uint64_t waves_per_block = kStageThreads / kWave;
            const unsigned sgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((N + waves_per_block - 1) / waves_per_block, (uint64_t)std::max(1, ctx->num_cu) * 16));
            hipLaunchKernelGGL(k_mreach_core, dim3(sgrid), dim3(kStageThreads), 0, stream, adj.p, aoff.p, N, k, core_w.p, core_e.p);
            hipLaunchKernelGGL(k_mreach_weights, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, core_w.p);
            RK_HIP(ctx, hipGetLastError());
            uint32_t most_h = 0;
            if (int r = rk_read_back(ctx, &most_h, most.p, 4, stream)) return r;   // (the entries and core_w[] go back to the pool behind this)
            st.max_degree = most_h;
        }
        // Boruvka rounds over the weights; the host reads one counter per round
        const uint64_t forest_cap = N - 1;
        uint32_t max_rounds = 2;   // 2 + ceil(log2 N): the components with an edge left at least halve per round, the last round appends nothing
        while ((1ULL << (max_rounds - 2)) < N) max_rounds++;
        DevBuf<uint32_t> parent(ctx), label(ctx);
        DevBuf<unsigned long long> best_w(ctx), best_rc(ctx), n_forest_dev(ctx), forest_w(ctx);
        DevBuf<rk_hit> forest(ctx);
        RK_HIP(ctx, parent.alloc(N));
        RK_HIP(ctx, label.alloc(N));
        RK_HIP(ctx, best_w.alloc(N));
        RK_HIP(ctx, best_rc.alloc(N));
        RK_HIP(ctx, n_forest_dev.alloc(1));
        RK_HIP(ctx, forest.alloc(forest_cap));
        RK_HIP(ctx, forest_w.alloc(forest_cap));
        RK_HIP(ctx, hipMemsetAsync(n_forest_dev.p, 0, 8, stream));
        hipLaunchKernelGGL(k_forest_init, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, parent.p, label.p, best_w.p, best_rc.p, N);
        RK_HIP(ctx, hipGetLastError());
        const rk_hit *hits = stage.hits.p;
        const unsigned long long *n_hits_dev = stage.cnt() + kCntHits, cap = stage.cap;
        unsigned long long n_forest = 0;
        for (bool settled = false; !settled;) {
            if (st.rounds == max_rounds) return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: %u rounds did not settle the forest of %u genomes (internal error)", max_rounds, N);
            hipLaunchKernelGGL(k_forest_match_w, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_hits_dev, cap, label.p, best_w.p);
            hipLaunchKernelGGL(k_forest_match_rc, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_hits_dev, cap, label.p, best_w.p, best_rc.p);
            hipLaunchKernelGGL(k_forest_link, dim3(grid), dim3(kStageThreads), 0, stream, hits, w.p, rc_.p, n_hits_dev, cap, label.p, best_w.p, best_rc.p, parent.p,
                               forest.p, (unsigned long long)forest_cap, n_forest_dev.p, forest_w.p);
            hipLaunchKernelGGL(k_forest_flatten, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, parent.p, label.p, best_w.p, best_rc.p, N);
            RK_HIP(ctx, hipGetLastError());
            unsigned long long now = 0;
            if (int r = rk_read_back(ctx, &now, n_forest_dev.p, 8, stream)) return r;
            st.rounds++;
            if (now > forest_cap) return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: %llu forest records for %u genomes (internal error)", now, N);
            settled = now == n_forest;
            n_forest = now;
        }
        RK_HIP(ctx, span.end());
        // the forest in order: by (row, col), then stably by the stored mw
        forest_h.resize(n_forest);
        if (n_forest) {
            DevBuf<rk_hit> tmp(ctx);
            DevBuf<unsigned long long> keys(ctx), keys_out(ctx);
            if (tmp.alloc(n_forest) != hipSuccess || keys.alloc(n_forest) != hipSuccess || keys_out.alloc(n_forest) != hipSuccess)
                return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate the sort buffers of %llu forest records", n_forest);
            const unsigned sgrid = (unsigned)((n_forest + kStageThreads - 1) / kStageThreads);
            hipLaunchKernelGGL(k_mreach_sort_keys, dim3(sgrid), dim3(kStageThreads), 0, stream, forest.p, forest_w.p, n_forest, 0, keys.p);
            RK_HIP(ctx, hipGetLastError());
            if (int r = rk_prim_sort_hits(ctx, keys.p, keys_out.p, forest.p, tmp.p, n_forest, 64, stream)) return rk_fail(ctx, r, "sorting the forest records failed");
            hipLaunchKernelGGL(k_mreach_sort_keys, dim3(sgrid), dim3(kStageThreads), 0, stream, tmp.p, forest_w.p, n_forest, 1, keys.p);
            RK_HIP(ctx, hipGetLastError());
            if (int r = rk_prim_sort_hits(ctx, keys.p, keys_out.p, tmp.p, forest.p, n_forest, 64, stream)) return rk_fail(ctx, r, "sorting the forest records failed");
            RK_HIP(ctx, hipMemcpyAsync(forest_h.data(), forest.p, n_forest * sizeof(rk_hit), hipMemcpyDeviceToHost, stream));
        }
        DevBuf<rk_hit> core_rec(ctx);
        if (k) {
            RK_HIP(ctx, core_rec.alloc(N));
            core_h.resize(N);
            hipLaunchKernelGGL(k_mreach_gather, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, hits, core_e.p, n_rec, N, core_rec.p);
            RK_HIP(ctx, hipGetLastError());
            RK_HIP(ctx, hipMemcpyAsync(core_h.data(), core_rec.p, (size_t)N * sizeof(rk_hit), hipMemcpyDeviceToHost, stream));
        }
        RK_HIP(ctx, hipStreamSynchronize(stream));
        span.read();
    }
    // the reference's values bit for bit (a record that took part lies below the exact threshold: none is dropped)
    const uint64_t n_forest = forest_h.size();
    for (const rk_hit &h : forest_h)
        if (h.row >= N || h.col >= N || h.row == h.col) return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: a forest record names a genome beyond the index (internal error)");
    if (rk_host_exact_distances(forest_h.data(), n_forest, opts) != n_forest)
        return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: a linked record lies beyond the exact threshold (internal error)");
    if (kruskal_sorted(forest_h.data(), n_forest, N) != n_forest) return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: the device's forest holds a cycle (internal error)");
    // the core records: those that exist, compacted, through the same routine, and back to their genomes
    for (uint32_t v = 0; v < N; v++) {
        core_dist_out[v] = k ? inf : 0.0;
        if (core_nb_out) core_nb_out[v] = kNone;
    }
    if (k && !core_h.empty()) {
        std::vector<uint32_t> owner;
        std::vector<rk_hit> have;
        for (uint32_t v = 0; v < N; v++) {
            const rk_hit &h = core_h[v];
            if (h.row == kNone && h.col == kNone) continue;
            if (h.row >= N || h.col >= N || h.row == h.col || (h.row != v && h.col != v))
                return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: the core record of genome %u is not incident to it (internal error)", v);
            owner.push_back(v);
            have.push_back(h);
        }
        if (rk_host_exact_distances(have.data(), have.size(), opts) != have.size())
            return rk_fail(ctx, RK_ERR_HIP, "rk_mreach_rows: a core record lies beyond the exact threshold (internal error)");
        for (size_t i = 0; i < owner.size(); i++) {
            core_dist_out[owner[i]] = have[i].dist;
            if (core_nb_out) core_nb_out[owner[i]] = other_end(have[i], owner[i]);
        }
        st.n_core = (uint32_t)owner.size();
    }
    if (!k) st.n_core = N;
    if (hand_over_edges(forest_h, edges_out, n_edges)) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu forest records failed", (unsigned long long)n_forest);
    st.n_trees = N - (uint32_t)n_forest;
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
