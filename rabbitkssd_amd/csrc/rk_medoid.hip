// rk_medoid.hip -- medoids and census of a clustering of `alldist` on the device (rk_medoid_rows), the same rule on the host over a hit
// list the caller already has (rk_medoid_hits), the fold of two disjoint record sets (rk_medoid_merge) and the per-cluster pick
// (rk_medoid_pick).  The graph is that of rk_cluster_rows; labels[v] < N names v's cluster, RK_MEDOID_NONE leaves v unlabelled.  A
// record (a, b) is INSIDE iff labels[a] == labels[b] != NONE, else LEAVING for both ends.  Per genome: in_deg, out_deg, central = the
// sum of q = floor(common * 2^32 / u) over its inside records, far_in = its inside record of the smallest ratio, near_out = its leaving
// record of the largest ratio (exact ratios, ties to the smaller neighbour index).  include/rabbitkssd.h, medoids and census.
//
//   stage     rk_edge_stage.h: the self join into a device buffer, its key pass (EdgeStage::key_pass<true>: per record w and
//             row << 32 | col; a BORDERLINE record goes, with its slot number, to the small host buffer and is dead for now; a record
//             outside 0 < common <= u -- multisets -- is counted: the call refuses such a collection), the two retries;
//   host      the stage decides the borderline records BEFORE anything is summed; the slot numbers of the kept ones go back up and
//             k_edge_revive gives them their keys.  The labels went up once, before the join (4 N bytes);
//   sums      k_medoid_sums, one sweep: per live record two label loads; inside -> atomic adds on in_deg and on central (q = ~w >> 30:
//             the staged key floor(c * 2^62 / u) shifted, no division) at both ends and the atomic MAXIMUM of w at both ends (far_w:
//             the largest w is the smallest ratio); leaving -> atomic adds on out_deg and the atomic MINIMUM of w at both ends (near_w);
//   settle    k_medoid_settle, one sweep: among the records that match a genome's far_w (inside) or near_w (leaving), the atomic minimum
//             of the neighbour's index (far_nb, near_nb) -- the two steps of k_dbscan_border, for two arrays;
//   gather    k_medoid_gather, one sweep: the record that matches (far_w, far_nb) or (near_w, near_nb) of an end is copied to that
//             end's entry: one pair is one record, so every entry has exactly one writer.  settle and gather are skipped when the
//             caller asks for no record array;
//   host      central, degrees and records are the tail of the stage's counter block: one read-back of 16 N (96 N with the records)
//             + 32 bytes, never O(hits); jorc and dist of the records are recomputed with the C library's log.
//
// Memory scope: w[], rc[], label[], far_w[], near_w[], far_nb[], near_nb[] are written by one kernel (or copy) and read by a later one
// on the same stream (plain accesses behind kernel boundaries: the settle sweep reads far_w / near_w plainly, the gather those and the
// two index arrays).  All communication INSIDE a kernel is relaxed agent-scope integer atomics (the eight XCDs have L2s of their own)
// whose result does not depend on arrival order: integer adds, a maximum, minima.  No loop waits for another workgroup, there are no
// barriers: any grid works.  DESIGN.md 4.12.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_edge_order.h"
#include "rk_edge_stage.h"
#include "rk_query_dev.h"

namespace {

constexpr uint32_t kNone = RK_MEDOID_NONE;
static_assert(sizeof(rk_hit) == 40 && sizeof(rk_medoid_cluster) == 112 && sizeof(rk_medoid_stats) == 48, "the layouts of include/rabbitkssd.h");

// where the results of n genomes lie in the tail: central (u64), the two degrees (u32 each), then -- with records -- far_in and near_out
struct Tail {
    unsigned long long *central;
    uint32_t *in_deg, *out_deg;
    rk_hit *far_in, *near_out;
    Tail(void *base, uint32_t n)
        : central((unsigned long long *)base), in_deg((uint32_t *)(central + n)), out_deg(in_deg + n), far_in((rk_hit *)(out_deg + n)), near_out(far_in + n) {}
    static size_t bytes(uint32_t n, bool records) { return (size_t)n * (records ? 16 + 2 * sizeof(rk_hit) : 16); }
};

__host__ __device__ inline rk_hit absent_record()
{
    return rk_hit{kNone, kNone, 0, 0, 0, 0, 0.0, 0.0};
}

__device__ __forceinline__ void max_u64(unsigned long long *p, unsigned long long v)
{
    // (as min_u64: the values only rise, a stale load costs an atomic, nothing else)
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// records: far_in / near_out may be null (no record array asked for)
__global__ void k_medoid_init(unsigned long long *far_w, unsigned long long *near_w, uint32_t *far_nb, uint32_t *near_nb, rk_hit *far_in, rk_hit *near_out, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        far_w[i] = 0;   // (w of a live record is ~key >= ~2^62 > 0)
        near_w[i] = kDead;
        far_nb[i] = kNone;
        near_nb[i] = kNone;
        if (far_in) {
            far_in[i] = absent_record();
            near_out[i] = absent_record();
        }
    }
}

// One sweep over the keyed records: the degrees, the sums and the two extreme keys of both ends.  (A wave-level combine of the lanes
// that share their row endpoint was tried and taken out again: DESIGN.md 4.12.)
__global__ void __launch_bounds__(kStageThreads)
k_medoid_sums(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *label, uint32_t *in_deg, uint32_t *out_deg,
              unsigned long long *central, unsigned long long *far_w, unsigned long long *near_w, int records)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t a = (uint32_t)(p >> 32), b = (uint32_t)p;
        const uint32_t la = label[a], lb = label[b];
        if (la == lb && la != kNone) {
            const unsigned long long q = ~we >> 30;   // floor(floor(c * 2^62 / u) / 2^30) = floor(c * 2^32 / u)
            add_u32(in_deg + a, 1u);
            add_u32(in_deg + b, 1u);
            add_u64(central + a, q);
            add_u64(central + b, q);
            if (records) {
                max_u64(far_w + a, we);
                max_u64(far_w + b, we);
            }
        } else {
            add_u32(out_deg + a, 1u);
            add_u32(out_deg + b, 1u);
            if (records) {
                min_u64(near_w + a, we);
                min_u64(near_w + b, we);
            }
        }
    }
}

// far_w[] and near_w[] are final: among the records that match an end's extreme the smallest neighbour wins
__global__ void __launch_bounds__(kStageThreads)
k_medoid_settle(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *label, const unsigned long long *far_w,
                const unsigned long long *near_w, uint32_t *far_nb, uint32_t *near_nb)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t a = (uint32_t)(p >> 32), b = (uint32_t)p;
        const uint32_t la = label[a], lb = label[b];
        const bool inside = la == lb && la != kNone;
        const unsigned long long *best = inside ? far_w : near_w;
        uint32_t *nb = inside ? far_nb : near_nb;
        if (best[a] == we) __hip_atomic_fetch_min(nb + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (best[b] == we) __hip_atomic_fetch_min(nb + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// far_nb[] and near_nb[] are final.  A pair is one record: the entry of an end has one writer
__global__ void __launch_bounds__(kStageThreads)
k_medoid_gather(const rk_hit *hits, const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *label,
                const unsigned long long *far_w, const unsigned long long *near_w, const uint32_t *far_nb, const uint32_t *near_nb, rk_hit *far_in, rk_hit *near_out)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t a = (uint32_t)(p >> 32), b = (uint32_t)p;
        const uint32_t la = label[a], lb = label[b];
        const bool inside = la == lb && la != kNone;
        const unsigned long long *best = inside ? far_w : near_w;
        const uint32_t *nb = inside ? far_nb : near_nb;
        rk_hit *out = inside ? far_in : near_out;
        const bool at_a = best[a] == we && nb[a] == b, at_b = best[b] == we && nb[b] == a;
        if (!at_a && !at_b) continue;
        rk_hit h = hits[e];
        h.pad_ = 0;
        if (at_a) out[a] = h;
        if (at_b) out[b] = h;
    }
}

// ---- host: the rule, exactly ------------------------------------------------------------------------------------------------
struct Genomes {   // the per-genome results, owned
    std::vector<uint32_t> in_deg, out_deg;
    std::vector<uint64_t> central;
    std::vector<rk_hit> far_in, near_out;
    explicit Genomes(uint32_t n) : in_deg(n, 0), out_deg(n, 0), central(n, 0), far_in(n, absent_record()), near_out(n, absent_record()) {}
};

inline bool present(const rk_hit &h) { return h.row != kNone; }

// a's ratio against b's by cross-multiplication: -1 smaller, 0 equal, 1 larger (both records have 0 < common <= u)
inline int ratio_cmp(const rk_hit &a, const rk_hit &b, int metric)
{
    long long ca, ua, cb, ub;
    ratio_terms(a.common, a.size0, a.size1, metric, &ca, &ua);
    ratio_terms(b.common, b.size0, b.size1, metric, &cb, &ub);
    const __int128 l = (__int128)ca * ub, r = (__int128)cb * ua;
    return l < r ? -1 : l > r ? 1 : 0;
}

// x replaces the present or absent `best` in v's entry: far (the smaller ratio wins) or near (the larger), ties to the smaller neighbour
inline bool takes_over(const rk_hit &x, const rk_hit &best, uint32_t v, int metric, bool far)
{
    if (!present(best)) return true;
    const int c = ratio_cmp(x, best, metric);
    if (c) return far ? c < 0 : c > 0;
    return other_end(x, v) < other_end(best, v);
}

inline rk_hit row_first(rk_hit h)
{
    if (h.row > h.col) {
        std::swap(h.row, h.col);
        std::swap(h.size0, h.size1);
    }
    return h;
}

int check_labels(const uint32_t *labels, uint32_t n)
{
    for (uint32_t v = 0; v < n; v++)
        if (labels[v] >= n && labels[v] != kNone) return RK_ERR_ARG;
    return RK_OK;
}

// what every entry point asks of the caller's arrays
inline bool has_sums(const rk_medoid_genomes *g) { return g && g->in_deg && g->out_deg && g->central; }

// the rule over a hit list; RK_ERR_ARG / RK_ERR_UNSUPPORTED as rk_medoid_hits answers them (labels are checked by the caller)
int medoid_of_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, const uint32_t *labels, int metric, Genomes *r)
{
    for (uint64_t e = 0; e < n_hits; e++) {
        const rk_hit &h = hits[e];
        if (h.row >= n || h.col >= n || h.row == h.col) return RK_ERR_ARG;
    }
    for (uint64_t e = 0; e < n_hits; e++) {
        long long c, u;
        ratio_terms(hits[e].common, hits[e].size0, hits[e].size1, metric, &c, &u);
        if (!(c > 0 && c <= u)) return RK_ERR_UNSUPPORTED;
    }
    for (uint64_t e = 0; e < n_hits; e++) {
        const rk_hit h = row_first(hits[e]);
        long long c, u;
        ratio_terms(h.common, h.size0, h.size1, metric, &c, &u);
        const uint64_t q = (uint64_t)(((unsigned __int128)c << 32) / (unsigned __int128)u);
        const bool inside = labels[h.row] == labels[h.col] && labels[h.row] != kNone;
        for (uint32_t v : {h.row, h.col}) {
            if (inside) {
                r->in_deg[v]++;
                r->central[v] += q;
                if (takes_over(h, r->far_in[v], v, metric, true)) r->far_in[v] = h;
            } else {
                r->out_deg[v]++;
                if (takes_over(h, r->near_out[v], v, metric, false)) r->near_out[v] = h;
            }
        }
    }
    return RK_OK;
}

void hand_over(const Genomes &r, uint32_t n, rk_medoid_genomes *out)
{
    if (!n) return;
    memcpy(out->in_deg, r.in_deg.data(), (size_t)n * 4);
    memcpy(out->out_deg, r.out_deg.data(), (size_t)n * 4);
    memcpy(out->central, r.central.data(), (size_t)n * 8);
    if (out->far_in) memcpy(out->far_in, r.far_in.data(), (size_t)n * sizeof(rk_hit));
    if (out->near_out) memcpy(out->near_out, r.near_out.data(), (size_t)n * sizeof(rk_hit));
}

// a present record of genome v's entry is a pair of v and another genome below n, row first
inline bool entry_ok(const rk_hit &h, uint32_t v, uint32_t n)
{
    return !present(h) ? h.col == kNone : (h.row < h.col && h.col < n && (h.row == v || h.col == v));
}

// jorc and dist of the present records of an array with the C library's log (a record that took part lies below the exact threshold:
// none is dropped); false when one was
bool exact_values(rk_hit *rec, uint32_t n, const rk_dist_opts *opts)
{
    std::vector<rk_hit> some;
    for (uint32_t v = 0; v < n; v++)
        if (present(rec[v])) some.push_back(rec[v]);
    if (rk_host_exact_distances(some.data(), some.size(), opts) != some.size()) return false;
    size_t k = 0;
    for (uint32_t v = 0; v < n; v++)
        if (present(rec[v])) rec[v] = some[k++];
    return true;
}

}  // namespace

extern "C" {

int rk_medoid_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, const uint32_t *labels, int metric, rk_medoid_genomes *out)
{
    if (!out || (n_hits && !hits) || (n && (!labels || !has_sums(out)))) return RK_ERR_ARG;
    if (n > (1u << 31)) return RK_ERR_UNSUPPORTED;
    if (int rc = check_labels(labels, n)) return rc;
    Genomes r(n);
    if (int rc = medoid_of_hits(hits, n_hits, n, labels, metric != 0, &r)) return rc;
    hand_over(r, n, out);
    return RK_OK;
}

int rk_medoid_merge(const rk_medoid_genomes *a, const rk_medoid_genomes *b, uint32_t n, int metric, rk_medoid_genomes *out)
{
    if (!a || !b || !out) return RK_ERR_ARG;
    if (!n) return RK_OK;
    if (!has_sums(a) || !has_sums(b) || !has_sums(out)) return RK_ERR_ARG;
    const bool far = a->far_in && b->far_in && out->far_in, near = a->near_out && b->near_out && out->near_out;
    for (uint32_t v = 0; v < n; v++) {
        if (far && (!entry_ok(a->far_in[v], v, n) || !entry_ok(b->far_in[v], v, n))) return RK_ERR_ARG;
        if (near && (!entry_ok(a->near_out[v], v, n) || !entry_ok(b->near_out[v], v, n))) return RK_ERR_ARG;
    }
    metric = metric != 0;
    for (uint32_t v = 0; v < n; v++) {   // (entry by entry: out may be a)
        out->in_deg[v] = a->in_deg[v] + b->in_deg[v];
        out->out_deg[v] = a->out_deg[v] + b->out_deg[v];
        out->central[v] = a->central[v] + b->central[v];
        if (far) {
            const rk_hit x = a->far_in[v], y = b->far_in[v];
            out->far_in[v] = present(y) && takes_over(y, x, v, metric, true) ? y : x;
        }
        if (near) {
            const rk_hit x = a->near_out[v], y = b->near_out[v];
            out->near_out[v] = present(y) && takes_over(y, x, v, metric, false) ? y : x;
        }
    }
    return RK_OK;
}

int rk_medoid_pick(const uint32_t *labels, const rk_medoid_genomes *g, uint32_t n, int metric, rk_medoid_cluster **out, uint32_t *n_out)
{
    if (!out || !n_out || !g) return RK_ERR_ARG;
    if (n && (!labels || !has_sums(g))) return RK_ERR_ARG;
    if (int rc = check_labels(labels, n)) return rc;
    *out = nullptr;
    *n_out = 0;
    if (!n) return RK_OK;
    metric = metric != 0;
    const bool records = g->far_in && g->near_out;
    std::vector<uint32_t> at(n, kNone);   // label -> its place among the non-empty clusters
    uint32_t count = 0;
    {
        std::vector<uint8_t> used(n, 0);
        for (uint32_t v = 0; v < n; v++)
            if (labels[v] != kNone) used[labels[v]] = 1;
        for (uint32_t l = 0; l < n; l++)
            if (used[l]) at[l] = count++;
    }
    if (!count) return RK_OK;
    rk_medoid_cluster *c = (rk_medoid_cluster *)calloc(count, sizeof(rk_medoid_cluster));
    if (!c) return RK_ERR_NOMEM;
    for (uint32_t l = 0; l < n; l++)
        if (at[l] != kNone) {
            c[at[l]].label = l;
            c[at[l]].medoid = kNone;
            c[at[l]].weakest_in = c[at[l]].nearest_out = absent_record();
        }
    const EdgeLess nearer{metric};
    for (uint32_t v = 0; v < n; v++) {   // ascending: at equal central the first member stays
        if (labels[v] == kNone) continue;
        rk_medoid_cluster &k = c[at[labels[v]]];
        k.size++;
        k.in_edges += g->in_deg[v];
        if (k.medoid == kNone || g->central[v] > k.central) {
            k.medoid = v;
            k.central = g->central[v];
        }
        if (!records) continue;
        const rk_hit &f = g->far_in[v], &o = g->near_out[v];
        if (present(f)) {
            const int cmp = present(k.weakest_in) ? ratio_cmp(f, k.weakest_in, metric) : -1;
            if (cmp < 0 || (!cmp && (f.row != k.weakest_in.row ? f.row < k.weakest_in.row : f.col < k.weakest_in.col))) k.weakest_in = f;
        }
        if (present(o) && (!present(k.nearest_out) || nearer(o, k.nearest_out))) k.nearest_out = o;
    }
    for (uint32_t i = 0; i < count; i++) c[i].in_edges /= 2;
    *out = c;
    *n_out = count;
    return RK_OK;
}

int rk_medoid_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, const uint32_t *labels, rk_medoid_genomes *out, rk_medoid_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_medoid_stats st;
    memset(&st, 0, sizeof st);
    const uint32_t N = idx->n_ref;
    if (!out) return rk_fail(ctx, RK_ERR_ARG, "rk_medoid_rows: out is null");
    if (N && !labels) return rk_fail(ctx, RK_ERR_ARG, "rk_medoid_rows: labels is null");
    if (N && !has_sums(out)) return rk_fail(ctx, RK_ERR_ARG, "rk_medoid_rows: in_deg, out_deg or central of out is null");
    const StageNeeds needs{"rk_medoid_rows", nullptr, true};
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    if (!N) {
        if (stats) *stats = st;
        return RK_OK;
    }
    if (N > (1u << 31)) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_medoid_rows: more than 2^31 genomes");
    if (check_labels(labels, N)) return rk_fail(ctx, RK_ERR_ARG, "rk_medoid_rows: a label is neither below the number of genomes nor RK_MEDOID_NONE");
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
    const TimedSpan span{ctx, RK_MS_MEDOID};
    span.clear();
    const bool records = out->far_in || out->near_out;

    // the same rule over the hit list on the host: the A/B leg of tools/medoid_probe.py, and a fallback
    if (rk_switched_off("RK_MEDOID_DEVICE")) {
        rk_hit *hits = nullptr;
        uint64_t n_hits = 0;
        if (int rc = rk_dist_rows(ctx, idx, nullptr, opts, &hits, &n_hits, nullptr)) return rc;
        Genomes r(N);
        const int rc = medoid_of_hits(hits, n_hits, N, labels, opts->metric != 0, &r);
        rk_free_host(hits);
        if (rc) return rk_fail(ctx, rc == RK_ERR_ARG ? RK_ERR_HIP : rc, "rk_medoid_rows: hit records lie outside 0 < common <= u (sketches that repeat hashes) or name a genome beyond the index");
        hand_over(r, N, out);
        st.edges = n_hits;
        for (uint32_t v = 0; v < N; v++) {
            st.inside += r.in_deg[v];
            st.leaving += r.out_deg[v];
        }
        st.inside /= 2;
        st.leaving /= 2;
        if (stats) *stats = st;
        return RK_OK;
    }

    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassGreedyKeys, Tail::bytes(N, records));   // with slot numbers; the tail: the results
    stage.tail_in_pass = false;   // (the key pass writes none of them)
    DevBuf<unsigned long long> w(ctx), rc_(ctx), far_w(ctx), near_w(ctx);
    DevBuf<uint32_t> label(ctx), far_nb(ctx), near_nb(ctx);
    RK_HIP(ctx, label.alloc(N));
    RK_HIP(ctx, far_w.alloc(N));
    RK_HIP(ctx, near_w.alloc(N));
    RK_HIP(ctx, far_nb.alloc(N));
    RK_HIP(ctx, near_nb.alloc(N));
    // the labels, once (pageable memory of the caller: the stage's first read-back synchronises the stream before this call returns)
    RK_HIP(ctx, hipMemcpyAsync(label.p, labels, (size_t)N * 4, hipMemcpyHostToDevice, stream));

    // the key pass: nothing is summed before the stage is through
    int rc = stage.run([&](int pass) { return stage.key_pass<true>(pass, w, rc_); });
    if (rc) return rc;
    stage.stats(&st);
    // the borderline records, decided before any sum
    if ((rc = stage.revive(w.p, &st.borderline_kept))) return rc;
    const unsigned long long n_rec = stage.n_hits;
    const unsigned grid = grid_for(ctx, n_rec), vgrid = grid_for(ctx, N);
    const Tail dev(stage.tail(), N);
    RK_HIP(ctx, hipMemsetAsync(dev.central, 0, (size_t)N * 16, stream));   // central and both degrees
    hipLaunchKernelGGL(k_medoid_init, dim3(vgrid), dim3(kStageThreads), 0, stream, far_w.p, near_w.p, far_nb.p, near_nb.p, records ? dev.far_in : (rk_hit *)nullptr,
                       records ? dev.near_out : (rk_hit *)nullptr, N);
    RK_HIP(ctx, hipGetLastError());
    RK_HIP(ctx, span.begin());
    hipLaunchKernelGGL(k_medoid_sums, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, label.p, dev.in_deg, dev.out_deg, dev.central, far_w.p, near_w.p,
                       (int)records);
    if (records) {
        hipLaunchKernelGGL(k_medoid_settle, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, label.p, far_w.p, near_w.p, far_nb.p, near_nb.p);
        hipLaunchKernelGGL(k_medoid_gather, dim3(grid), dim3(kStageThreads), 0, stream, stage.hits.p, w.p, rc_.p, n_rec, label.p, far_w.p, near_w.p, far_nb.p,
                           near_nb.p, dev.far_in, dev.near_out);
    }
    RK_HIP(ctx, hipGetLastError());
    RK_HIP(ctx, span.end());
    if ((rc = stage.fetch_home())) return rc;
    span.read();
    const Tail home((void *)stage.home_tail(), N);
    unsigned long long in_sum = 0, out_sum = 0;
    for (uint32_t v = 0; v < N; v++) {
        in_sum += home.in_deg[v];
        out_sum += home.out_deg[v];
    }
    const unsigned long long live = n_rec - stage.n_border + st.borderline_kept;
    if (in_sum + out_sum != 2 * live)
        return rk_fail(ctx, RK_ERR_HIP, "rk_medoid_rows: the degrees of %u genomes do not add up to the records (internal error)", N);
    if (records) {   // the reference's values bit for bit, in the scratch (nothing of the caller's is written before every check is through)
        for (uint32_t v = 0; v < N; v++)
            if (!entry_ok(home.far_in[v], v, N) || !entry_ok(home.near_out[v], v, N) || present(home.far_in[v]) != (home.in_deg[v] != 0) ||
                present(home.near_out[v]) != (home.out_deg[v] != 0))
                return rk_fail(ctx, RK_ERR_HIP, "rk_medoid_rows: the records of genome %u do not match its degrees (internal error)", v);
        if (!exact_values(home.far_in, N, opts) || !exact_values(home.near_out, N, opts))
            return rk_fail(ctx, RK_ERR_HIP, "rk_medoid_rows: a record lies beyond the exact threshold (internal error)");
    }
    memcpy(out->in_deg, home.in_deg, (size_t)N * 4);
    memcpy(out->out_deg, home.out_deg, (size_t)N * 4);
    memcpy(out->central, home.central, (size_t)N * 8);
    if (out->far_in) memcpy(out->far_in, home.far_in, (size_t)N * sizeof(rk_hit));
    if (out->near_out) memcpy(out->near_out, home.near_out, (size_t)N * sizeof(rk_hit));
    st.inside = in_sum / 2;
    st.leaving = out_sum / 2;
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
