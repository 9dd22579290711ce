// rk_knn.hip -- the k nearest neighbours of every genome within -D, the kNN graph of `alldist`, on the device (rk_knn_rows), and
// its host side: the same lists from a hit list the caller already has (rk_knn_hits) and the fold of two results (rk_knn_merge).
// The graph is that of rk_cluster_rows.  A record is incident to its row and to its col; the list of genome v holds the first
// min(k, degree(v)) records incident to v in the order of rk_edge_order.h restricted to v: the ratio common / u descending, compared
// exactly, then the NEIGHBOUR's caller index ascending (the (row, col) tie-break of EdgeLess with one endpoint fixed).
//
//   stage     rk_edge_stage.h: the self join into a device buffer, its key pass (EdgeStage::key_pass<false>: per record w and
//             row << 32 | col; a BORDERLINE record and a record outside 0 < common <= u -- multisets: no key -- go to the small host
//             buffer and are dead on the device), the two retries;
//   degree    k_edge_degree: per live record one atomicAdd on deg[row] and one on deg[col] -- behind the stage, whose pass may run twice;
//   (offsets, fill and the selection's body: rk_knn_select.h, shared with rk_mreach.hip)
//   offsets   k_knn_offsets writes min(deg, k) and the largest degree; two exclusive scans give the adjacency offsets aoff[] and the
//             output offsets koff[] (N + 1 words each);
//   fill      k_knn_fill: per live record and endpoint v the 16-byte entry {w, other << 32 | e} at aoff[v] + atomicAdd(cur + v, 1).
//             Entries compared as (first word, second word) ascending are exactly the order above (e < 2^31: more records fall
//             back).  The place inside a segment depends on the run, the selection's result does not;
//   select    k_knn_select: one wave64 per genome, the waves grid-striding over the genomes.  Lane l holds the l-th best entry so far
//             or (kDead, kDead); lanes >= k stay dead.  The segment streams in chunks of 64, one 16-byte load per lane; a ballot keeps
//             the candidates that beat the current k-th (lane k - 1); each survivor is broadcast, tested again against the tightened
//             k-th, ranked by the number of lanes that precede it and inserted with one shuffle up.  Lane l < min(deg, k) writes
//             hits[e] to out[koff[v] + l];
//   host      koff[] and the records come home (4 (N + 1) + 40 * sum of min(deg, k) bytes, never O(hits)), jorc / dist recomputed
//             with the C library's log; the stage's kept borderline records are folded into their two endpoints' lists with the
//             routine rk_knn_merge uses (a kept edge changes those two lists only).
//
// Memory scope: w[], rc[], deg[], aoff[], koff[], cur[] and the entries are written by one kernel and read by a later one on the same
// stream (plain accesses behind kernel boundaries).  The only communication inside a kernel is the relaxed agent-scope atomicAdds of
// the degree and the fill pass (and the atomicMax of the largest degree).  No loop waits for another workgroup, and k_knn_select has no
// barrier: the waves of a workgroup have different trip counts.  DESIGN.md 4.9.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_edge_order.h"
#include "rk_edge_stage.h"
#include "rk_knn_select.h"

namespace {

// 1 <= k <= 64: the selection of rk_knn_select.h, then lane l < min(deg, k) writes the record of its entry
__global__ void __launch_bounds__(kStageThreads)
k_knn_select(const KnnEntry *adj, const uint32_t *aoff, const uint32_t *koff, const rk_hit *hits, uint32_t n, uint32_t k, rk_hit *out)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t n_waves = (gridDim.x * blockDim.x) / kWave;
    for (uint32_t v = (blockIdx.x * blockDim.x + threadIdx.x) / kWave; v < n; v += n_waves) {
        const unsigned long long beg = aoff[v], end = aoff[v + 1];
        unsigned long long bw, bx;
        knn_select_wave(adj, beg, end, lane, k, &bw, &bx);
        if (lane < min((unsigned long long)k, end - beg)) out[koff[v] + lane] = hits[(uint32_t)bx];
    }
}

// `pool` (records incident to v, any order) -> its first k in the order, one record per neighbour
void first_k(std::vector<rk_hit> *pool, uint32_t v, uint64_t k, int metric)
{
    std::sort(pool->begin(), pool->end(), NeighbourLess{metric, v});
    size_t kept = 0;
    for (size_t i = 0; i < pool->size() && kept < k; i++)
        if (!kept || other_end((*pool)[kept - 1], v) != other_end((*pool)[i], v)) (*pool)[kept++] = (*pool)[i];
    pool->resize(kept);
}

bool in_order(const rk_hit *rec, uint64_t m, uint32_t v, int metric)
{
    for (uint64_t j = 1; j < m; j++)
        if (!NeighbourLess{metric, v}(rec[j - 1], rec[j])) return false;
    return true;
}

// offsets ascend from wherever they start, every record of list i is incident to i and names genomes below n
bool lists_valid(const uint64_t *off, const rk_hit *rec, uint32_t n)
{
    if (!off) return false;
    for (uint32_t i = 0; i < n; i++)   // (all offsets before any record: a record is read only inside ascending offsets)
        if (off[i] > off[i + 1]) return false;
    if (off[0] < off[n] && !rec) return false;
    for (uint32_t i = 0; i < n; i++)
        for (uint64_t at = off[i]; at < off[i + 1]; at++) {
            const rk_hit &h = rec[at];
            if (h.row >= n || h.col >= n || h.row == h.col || (h.row != i && h.col != i)) return false;
        }
    return true;
}

// per genome the first k of the union of two lists (validated by the caller)
void fold_lists(const uint64_t *a_off, const rk_hit *a, const uint64_t *b_off, const rk_hit *b, uint32_t n, uint64_t k, int metric,
                uint64_t *off_out, std::vector<rk_hit> *out)
{
    out->clear();
    std::vector<rk_hit> pool;
    off_out[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        // one side empty, the other within k and in (strict) order already: nothing to fold
        const uint64_t na = a_off[i + 1] - a_off[i], nb = b_off[i + 1] - b_off[i];
        const rk_hit *one = na ? a + a_off[i] : b + b_off[i];
        if ((!na || !nb) && na + nb <= k && in_order(one, na + nb, i, metric))
            out->insert(out->end(), one, one + na + nb);
        else {
            pool.assign(a + a_off[i], a + a_off[i + 1]);
            pool.insert(pool.end(), b + b_off[i], b + b_off[i + 1]);
            first_k(&pool, i, k, metric);
            out->insert(out->end(), pool.begin(), pool.end());
        }
        off_out[i + 1] = out->size();
    }
}

// the lists of a hit list (validated by the caller): its adjacency, then the first k of each genome's records
void lists_of_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint64_t k, int metric, uint64_t *off_out, std::vector<rk_hit> *out)
{
    std::vector<uint64_t> start, adj;
    hit_adjacency(hits, n_hits, n, &start, &adj);
    out->clear();
    std::vector<rk_hit> pool;
    off_out[0] = 0;
    for (uint32_t v = 0; v < n; v++) {
        pool.clear();
        for (uint64_t at = start[v]; at < start[v + 1]; at++) pool.push_back(hits[adj[at]]);
        first_k(&pool, v, k, metric);
        out->insert(out->end(), pool.begin(), pool.end());
        off_out[v + 1] = out->size();
    }
}

// records for the caller of the library: NULL when there is none
int hand_over(const std::vector<rk_hit> &rec, rk_hit **out, uint64_t *n_out)
{
    *out = nullptr;
    *n_out = rec.size();
    if (rec.empty()) return RK_OK;
    rk_hit *p = host_records(rec.size());
    if (!p) return RK_ERR_NOMEM;
    memcpy(p, rec.data(), rec.size() * sizeof(rk_hit));
    *out = p;
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_knn_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, uint32_t k, int metric, uint64_t *off_out, rk_hit **nbrs_out, uint64_t *n_nbrs)
{
    if ((n_hits && !hits) || !off_out || !nbrs_out || !n_nbrs) return RK_ERR_ARG;
    for (uint64_t e = 0; e < n_hits; e++)
        if (hits[e].row >= n || hits[e].col >= n || hits[e].row == hits[e].col) return RK_ERR_ARG;
    std::vector<rk_hit> rec;
    lists_of_hits(hits, n_hits, n, k, metric != 0, off_out, &rec);
    return hand_over(rec, nbrs_out, n_nbrs);
}

int rk_knn_merge(const uint64_t *a_off, const rk_hit *a, const uint64_t *b_off, const rk_hit *b, uint32_t n, uint32_t k, int metric,
                 uint64_t *off_out, rk_hit **out, uint64_t *n_out)
{
    if (!a_off || !b_off || !off_out || !out || !n_out) return RK_ERR_ARG;
    if (!lists_valid(a_off, a, n) || !lists_valid(b_off, b, n)) return RK_ERR_ARG;
    std::vector<uint64_t> off((size_t)n + 1);   // (off_out may be one of the inputs' offsets)
    std::vector<rk_hit> rec;
    fold_lists(a_off, a, b_off, b, n, k, metric != 0, off.data(), &rec);
    if (int rc = hand_over(rec, out, n_out)) return rc;
    memcpy(off_out, off.data(), off.size() * 8);
    return RK_OK;
}

int rk_knn_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, uint32_t k, uint64_t *off_out, rk_hit **nbrs_out, uint64_t *n_nbrs,
                rk_knn_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_knn_stats st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    if (!off_out || !nbrs_out || !n_nbrs) return rk_fail(ctx, RK_ERR_ARG, "off_out, nbrs_out or n_nbrs is null");
    *nbrs_out = nullptr;
    *n_nbrs = 0;
    const StageNeeds needs{"rk_knn_rows", nullptr, true};
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    const uint32_t N = idx->n_ref;
    std::fill(off_out, off_out + (size_t)N + 1, (uint64_t)0);
    if (!N) return RK_OK;
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
    if (!k) return RK_OK;
    const int metric = opts->metric != 0;

    // the same lists from the hit list on the host: what the device path has no room for
    auto on_the_host = [&]() -> int {
        rk_hit *hits = nullptr;
        uint64_t n_hits = 0;
        if (int rc = rk_dist_rows(ctx, idx, nullptr, opts, &hits, &n_hits, nullptr)) return rc;
        std::vector<rk_hit> rec;
        lists_of_hits(hits, n_hits, N, k, metric, off_out, &rec);
        rk_free_host(hits);
        if (hand_over(rec, nbrs_out, n_nbrs)) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu neighbour records failed", (unsigned long long)rec.size());
        memset(&st, 0, sizeof st);
        st.edges = n_hits;
        st.neighbours = rec.size();
        st.path = 2;
        if (stats) *stats = st;
        return RK_OK;
    };
    if (k > kKnnDeviceMax || (uint64_t)N * k >= (1ULL << 32) || rk_switched_off("RK_KNN_DEVICE")) return on_the_host();

    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassKeys);
    const TimedSpan span{ctx, RK_MS_KNN_SELECT};
    span.clear();
    DevBuf<unsigned long long> w(ctx), rc_(ctx);
    int rc = stage.run([&](int pass) { return stage.key_pass<false>(pass, w, rc_); });
    if (stage.beyond_31_bits(rc)) {   // the entries number the records in 31 bits
        w.reset();
        rc_.reset();
        return on_the_host();
    }
    if (rc) return rc;
    stage.stats(&st);
    st.path = 1;
    const unsigned long long n_rec = stage.n_hits, n_live = n_rec - stage.n_border;

    std::vector<uint64_t> off((size_t)N + 1, 0);
    std::vector<rk_hit> rec;
    if (n_live) {
        DevBuf<uint32_t> deg(ctx), kmin(ctx), aoff(ctx), koff(ctx), most(ctx);
        DevBuf<KnnEntry> adj(ctx);
        DevBuf<rk_hit> out(ctx);
        RK_HIP(ctx, deg.alloc((size_t)N + 1));
        RK_HIP(ctx, kmin.alloc((size_t)N + 1));
        RK_HIP(ctx, aoff.alloc((size_t)N + 1));
        RK_HIP(ctx, koff.alloc((size_t)N + 1));
        RK_HIP(ctx, most.alloc(1));
        const uint64_t n_out_max = std::min<uint64_t>((uint64_t)N * k, 2 * n_live);
        if (adj.alloc(2 * n_live) != hipSuccess || out.alloc(n_out_max) != hipSuccess)
            return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate the adjacency of %llu hit records on the device", n_live);
        const unsigned grid = grid_for(ctx, n_rec), vgrid = grid_for(ctx, (uint64_t)N + 1);
        RK_HIP(ctx, span.begin());
        RK_HIP(ctx, hipMemsetAsync(deg.p, 0, ((size_t)N + 1) * 4, stream));
        RK_HIP(ctx, hipMemsetAsync(most.p, 0, 4, stream));
        hipLaunchKernelGGL(k_edge_degree, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, deg.p);
        hipLaunchKernelGGL(k_knn_offsets, dim3(vgrid), dim3(kStageThreads), 0, stream, deg.p, kmin.p, N, k, most.p);
        RK_HIP(ctx, hipGetLastError());
        if (int r = rk_prim_exclusive_scan_u32(ctx, deg.p, aoff.p, (uint64_t)N + 1, stream)) return rk_fail(ctx, r, "rk_knn_rows: the scan of the degrees failed");
        if (int r = rk_prim_exclusive_scan_u32(ctx, kmin.p, koff.p, (uint64_t)N + 1, stream)) return rk_fail(ctx, r, "rk_knn_rows: the scan of the list lengths failed");
        RK_HIP(ctx, hipMemsetAsync(deg.p, 0, (size_t)N * 4, stream));   // from here on the cursors of the fill
        hipLaunchKernelGGL(k_knn_fill, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, aoff.p, deg.p, adj.p);
        const uint64_t waves_per_block = kStageThreads / kWave;
        const unsigned sgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((N + waves_per_block - 1) / waves_per_block, (uint64_t)std::max(1, ctx->num_cu) * 16));
        hipLaunchKernelGGL(k_knn_select, dim3(sgrid), dim3(kStageThreads), 0, stream, adj.p, aoff.p, koff.p, stage.hits.p, N, k, out.p);
        RK_HIP(ctx, hipGetLastError());
        RK_HIP(ctx, span.end());
        // koff[], then the records it counts
        std::vector<uint32_t> koff_h((size_t)N + 1);
        uint32_t most_h = 0;
        RK_HIP(ctx, hipMemcpyAsync(koff_h.data(), koff.p, koff_h.size() * 4, hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipMemcpyAsync(&most_h, most.p, 4, hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipStreamSynchronize(stream));
        span.read();
        st.max_degree = most_h;
        const uint64_t total = koff_h[N];
        if (total > n_out_max) return rk_fail(ctx, RK_ERR_HIP, "rk_knn_rows: %llu neighbour records where %llu are possible (internal error)", (unsigned long long)total, (unsigned long long)n_out_max);
        rec.resize(total);
        if (total) {
            RK_HIP(ctx, hipMemcpyAsync(rec.data(), out.p, total * sizeof(rk_hit), hipMemcpyDeviceToHost, stream));
            RK_HIP(ctx, hipStreamSynchronize(stream));
        }
        for (uint32_t i = 0; i <= N; i++) off[i] = koff_h[i];
        for (uint32_t i = 0; i < N; i++) {
            if (off[i] > off[i + 1] || off[i + 1] - off[i] > k) return rk_fail(ctx, RK_ERR_HIP, "rk_knn_rows: the list of genome %u is out of shape (internal error)", i);
            for (uint64_t at = off[i]; at < off[i + 1]; at++)
                if ((rec[at].row != i && rec[at].col != i) || rec[at].row >= N || rec[at].col >= N || rec[at].row == rec[at].col)
                    return rk_fail(ctx, RK_ERR_HIP, "rk_knn_rows: a record in the list of genome %u is not incident to it (internal error)", i);
        }
        // the reference's values bit for bit (a record that took part lies below the exact threshold: none is dropped)
        if (rk_host_exact_distances(rec.data(), total, opts) != total)
            return rk_fail(ctx, RK_ERR_HIP, "rk_knn_rows: a neighbour record lies beyond the exact threshold (internal error)");
    }
    // the borderline records the host keeps: their own lists, folded in
    {
        std::vector<rk_hit> kept;
        if ((rc = stage.decide(&kept))) return rc;
        st.borderline_kept = kept.size();
        if (!kept.empty()) {
            for (const rk_hit &h : kept)
                if (h.row >= N || h.col >= N || h.row == h.col) return rk_fail(ctx, RK_ERR_HIP, "rk_knn_rows: a borderline record names a genome beyond the index (internal error)");
            std::vector<uint64_t> b_off((size_t)N + 1), f_off((size_t)N + 1);
            std::vector<rk_hit> b, folded;
            lists_of_hits(kept.data(), kept.size(), N, k, metric, b_off.data(), &b);
            fold_lists(off.data(), rec.data(), b_off.data(), b.data(), N, k, metric, f_off.data(), &folded);
            off.swap(f_off);
            rec.swap(folded);
        }
    }
    if (hand_over(rec, nbrs_out, n_nbrs)) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu neighbour records failed", (unsigned long long)rec.size());
    memcpy(off_out, off.data(), off.size() * 8);
    st.neighbours = rec.size();
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
