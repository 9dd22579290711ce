// rk_assign.hip -- placement of query genomes into a labelled collection on the device (rk_assign_rows) and the same rule on the host
// over a hit list the caller already has (rk_assign_hits).  The graph is that of rk_dist_rows with explicit queries (triangle = 0,
// dist <= max_dist); labels[r] < N names reference r's cluster, RK_ASSIGN_NONE leaves r unlabelled.  Per query q: n_within (its
// records), n_labelled (those to a labelled reference), nearest (its record of the largest ratio among the labelled references, exact
// ratios, ties to the smaller reference index), label = the label of that reference (NONE: q is novel), n_same (its records to
// references of that label), runner_up (the nearest record among the references of OTHER labels).  include/rabbitkssd.h, placement.
//
//   stage     rk_edge_stage.h over the QUERY join (EdgeStage::queries): the join into a device buffer, its key pass with slot numbers
//             (k_assign_keys, k_edge_keys<true> with the bounds of a query join: per record w and row << 32 | col; a BORDERLINE record
//             goes, with its slot number, to the small host buffer and is dead for now; a record outside 0 < common <= u -- multisets --
//             is counted: the call refuses such a collection), the two retries;
//   host      the stage decides the borderline records (`<=`: triangle = 0) BEFORE anything is counted; the slot numbers of the kept ones
//             go back up and k_edge_revive gives them their keys.  The labels went up once, before the join (4 N bytes);
//   first     k_assign_first, one sweep: per live record one label load; atomic adds on n_within and, labelled, on n_labelled of its
//             query, and the atomic MINIMUM of w at its query (best_w: the smallest w is the largest ratio).  A wave whose live records
//             all belong to one query combines them first (ballots, a 6-step shuffle minimum) and lets one lane speak: measured, it
//             wins where a query has hundreds of references and costs nothing elsewhere (RK_ASSIGN_COMBINE=0: lane by lane);
//   settle    k_assign_settle<false>, one sweep: among the labelled records that match their query's best_w the atomic minimum of the
//             reference's index (best_nb) -- the two steps of k_dbscan_border;
//   label     k_assign_label, one thread per query: label[q] = labels[best_nb[q]];
//   second    k_assign_second, one sweep: the reference carries label[row] -> atomic add on n_same; labelled otherwise -> the atomic
//             minimum of w at the query (second_w; with a record array only);
//   settle    k_assign_settle<true> for second_nb, then k_assign_gather, one sweep: the record (row, best_nb[row]) is copied to
//             nearest[row], (row, second_nb[row]) to runner_up[row]: one pair is one record, so every entry has exactly one writer.
//             These two are skipped when the caller asks for no record array;
//   host      label, the three counts and the records are the tail of the stage's counter block: one read-back of 16 Q (96 Q with the
//             records) + 32 bytes, never O(hits); jorc and dist of the records are recomputed with the C library's log.  Only the
//             entries of the selected query rows are written.
//
// Memory scope: w[], rc[], dlabels[], best_w[], best_nb[], second_w[], second_nb[] and label[] are written by one kernel (or copy) and
// read by a later one on the same stream (plain accesses behind kernel boundaries: the settle sweeps read best_w / second_w plainly,
// the second sweep label[], the gather the index arrays).  All communication INSIDE a kernel is relaxed agent-scope integer atomics (the
// eight XCDs have L2s of their own) whose result does not depend on arrival order: integer adds and minima -- and, inside one wave,
// ballots and shuffles (registers, no memory; the two sweeps that use them keep whole waves together).  No loop waits for another
// workgroup, there are no barriers: any grid works.  DESIGN.md 4.13.
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

constexpr uint32_t kNone = RK_ASSIGN_NONE;
static_assert(sizeof(rk_hit) == 40 && sizeof(rk_assign_stats) == 48, "the layouts of include/rabbitkssd.h");

// where the results of q queries lie in the tail: label and the three counts (u32 each), then -- with records -- nearest and runner_up
struct Tail {
    uint32_t *label, *n_within, *n_labelled, *n_same;
    rk_hit *nearest, *runner_up;
    Tail(void *base, uint32_t q)
        : label((uint32_t *)base), n_within(label + q), n_labelled(n_within + q), n_same(n_labelled + q), nearest((rk_hit *)(n_same + q)), runner_up(nearest + q) {}
    static size_t bytes(uint32_t q, bool records) { return (size_t)q * (records ? 16 + 2 * sizeof(rk_hit) : 16); }
};

__host__ __device__ inline rk_hit absent_record()
{
    return rk_hit{kNone, kNone, 0, 0, 0, 0, 0.0, 0.0};
}

// records: nearest / runner_up may be null (no record array asked for).  label[] is written by k_assign_label, the counts by a memset
__global__ void k_assign_init(unsigned long long *best_w, unsigned long long *second_w, uint32_t *best_nb, uint32_t *second_nb, rk_hit *nearest, rk_hit *runner_up,
                              uint32_t q)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < q; i += gridDim.x * blockDim.x) {
        best_w[i] = kDead;
        second_w[i] = kDead;
        best_nb[i] = kNone;
        second_nb[i] = kNone;
        if (nearest) {
            nearest[i] = absent_record();
            runner_up[i] = absent_record();
        }
    }
}

// The key pass of the stage behind a QUERY join: k_edge_keys<true> of rk_edge_stage.h with the bounds of a query join -- row is a query
// below n_query, col a reference below n_ref, and row == col names two different sketches.  (A kernel of its own, so that the key pass
// of the seven self-join callers stays the code it was.)  Per record w and row << 32 | col; a borderline record goes to the host
// buffer with its slot number and is dead for now; a record outside 0 < common <= u is counted: the call refuses the collection.
__global__ void __launch_bounds__(kStageThreads)
k_assign_keys(const rk_hit *hits, unsigned long long *cnt, unsigned long long cap, uint32_t n_query, uint32_t n_ref, double link_below, int metric,
              unsigned long long *w_out, unsigned long long *rc_out, rk_edge *edges, unsigned long long *slots, unsigned long long edge_cap)
{
    const unsigned long long n_rec = min(cnt[kCntHits], cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const rk_hit h = hits[e];
        rc_out[e] = ((unsigned long long)h.row << 32) | h.col;
        long long c, u;
        ratio_terms(h.common, h.size0, h.size1, metric, &c, &u);
        const bool bad = h.row >= n_query || h.col >= n_ref;   // (never from the join's kernel; nothing is indexed by such a record)
        const bool keyed = c > 0 && c <= u;
        unsigned long long w = kDead;
        if (bad || !keyed) atomicAdd(cnt + (bad ? kCntBad : kCntRange), 1ULL);
        else if (!(h.dist < link_below)) edge_append(h, e, edges, slots, edge_cap, cnt + kCntBorder);
        else w = ~ratio_key((unsigned long long)c, (unsigned long long)u);   // (key >= 1: never kDead)
        w_out[e] = w;
    }
}

// pass k of EdgeStage::run, as EdgeStage::key_pass<true>: the buffers are the caller's, allocated at k = 0
int query_key_pass(EdgeStage &stage, int k, DevBuf<unsigned long long> &w, DevBuf<unsigned long long> &rc)
{
    rk_ctx *ctx = stage.ctx;
    if (!k && (w.alloc(stage.cap) != hipSuccess || rc.alloc(stage.cap) != hipSuccess))
        return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu %s on the device", (unsigned long long)stage.cap, stage.hits_what);
    hipLaunchKernelGGL(k_assign_keys, dim3(grid_for(ctx, stage.cap)), dim3(kStageThreads), 0, ctx->stream, stage.hits.p, stage.cnt(), (unsigned long long)stage.cap,
                       stage.n_rows, stage.idx->n_ref, stage.link_below, stage.metric, w.p, rc.p, stage.edges.p, stage.slots.p, (unsigned long long)stage.edge_cap);
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}

// the smallest v of the 64 lanes of a wave, in every lane (all 64 lanes take part: the callers' loops keep whole waves together)
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    for (int s = 32; s; s >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, s, 64));
    return v;
}

// the live lanes of a wave all carry one row: that row's first live lane may speak for them.  *leader: this lane is it
__device__ __forceinline__ bool wave_one_row(bool live, uint32_t row, bool *leader)
{
    const unsigned long long lanes = __ballot(live);
    if (!lanes) return *leader = false;
    const int first = __ffsll((long long)lanes) - 1;
    const uint32_t row0 = (uint32_t)__shfl((int)row, first, 64);
    *leader = (int)(threadIdx.x & 63) == first;
    return __ballot(live && row == row0) == lanes;
}

// One sweep over the keyed records: the two counts and the key of the nearest labelled reference of every query.  The loop is uniform
// for a workgroup (whole waves stay together).  COMBINE (RK_ASSIGN_COMBINE): a wave whose live records all belong to one
// query -- a query with hundreds of references within -D -- makes its two adds and its minimum once, not once per lane.
template <bool COMBINE>
__global__ void __launch_bounds__(kStageThreads)
k_assign_first(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *dlabels, uint32_t *n_within, uint32_t *n_labelled,
               unsigned long long *best_w)
{
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n_rec; base += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long e = base + threadIdx.x;
        const unsigned long long we = e < n_rec ? w[e] : kDead;
        const bool live = we != kDead;
        const unsigned long long p = live ? rc[e] : 0;
        const uint32_t row = (uint32_t)(p >> 32), col = (uint32_t)p;
        const bool labelled = live && dlabels[col] != kNone;
        bool leader = false;
        if (COMBINE && wave_one_row(live, row, &leader)) {
            const uint32_t all = (uint32_t)__popcll(__ballot(live)), some = (uint32_t)__popcll(__ballot(labelled));
            const unsigned long long best = wave_min_u64(labelled ? we : kDead);
            if (leader) {
                add_u32(n_within + row, all);
                if (some) {
                    add_u32(n_labelled + row, some);
                    min_u64(best_w + row, best);
                }
            }
            continue;
        }
        if (!live) continue;
        add_u32(n_within + row, 1u);
        if (!labelled) continue;
        add_u32(n_labelled + row, 1u);
        min_u64(best_w + row, we);
    }
}

// best_w[] (SECOND: second_w[]) is final: among the records that match their query's key the smallest reference wins.  SECOND looks
// at the labelled records whose label is not the query's, the first settle at every labelled record
template <bool SECOND, bool COMBINE>
__global__ void __launch_bounds__(kStageThreads)
k_assign_settle(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *dlabels, const uint32_t *label,
                const unsigned long long *key, uint32_t *nb)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t row = (uint32_t)(p >> 32), col = (uint32_t)p;
        if (key[row] != we) continue;
        const uint32_t l = dlabels[col];
        if (l == kNone || (SECOND && l == label[row])) continue;
        // (COMBINE: as min_u64 -- the values only fall, a stale load costs an atomic, nothing else)
        if (COMBINE && !(col < __hip_atomic_load(nb + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) continue;
        __hip_atomic_fetch_min(nb + row, col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// best_nb[] is final
__global__ void k_assign_label(const uint32_t *dlabels, const uint32_t *best_nb, uint32_t *label, uint32_t q)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < q; i += gridDim.x * blockDim.x) {
        const uint32_t nb = best_nb[i];
        label[i] = nb == kNone ? kNone : dlabels[nb];
    }
}

// label[] is final: the support, and -- records -- the key of the nearest reference of another label.  (The loop and COMBINE as in
// k_assign_first)
template <bool COMBINE>
__global__ void __launch_bounds__(kStageThreads)
k_assign_second(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *dlabels, const uint32_t *label, uint32_t *n_same,
                unsigned long long *second_w, int records)
{
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n_rec; base += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long e = base + threadIdx.x;
        const unsigned long long we = e < n_rec ? w[e] : kDead;
        const bool live = we != kDead;
        const unsigned long long p = live ? rc[e] : 0;
        const uint32_t row = (uint32_t)(p >> 32), col = (uint32_t)p;
        const uint32_t l = live ? dlabels[col] : kNone;
        const bool same = l != kNone && l == label[row], other = l != kNone && !same;   // (row 0 of a lane that is not live: label[0] is read, nothing follows)
        bool leader = false;
        if (COMBINE && wave_one_row(live, row, &leader)) {
            const uint32_t support = (uint32_t)__popcll(__ballot(same));
            const unsigned long long others = __ballot(other);
            const unsigned long long best = records ? wave_min_u64(other ? we : kDead) : kDead;
            if (leader) {
                if (support) add_u32(n_same + row, support);
                if (records && others) min_u64(second_w + row, best);
            }
            continue;
        }
        if (same) add_u32(n_same + row, 1u);
        else if (other && records) min_u64(second_w + row, we);
    }
}

// best_nb[] and second_nb[] are final.  A pair is one record: an entry has one writer
__global__ void __launch_bounds__(kStageThreads)
k_assign_gather(const rk_hit *hits, const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *best_nb,
                const uint32_t *second_nb, rk_hit *nearest, rk_hit *runner_up)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        if (w[e] == kDead) continue;
        const unsigned long long p = rc[e];
        const uint32_t row = (uint32_t)(p >> 32), col = (uint32_t)p;
        const bool first = best_nb[row] == col, second = second_nb[row] == col;   // (col < N: never kNone)
        if (!first && !second) continue;
        rk_hit h = hits[e];
        h.pad_ = 0;
        (first ? nearest : runner_up)[row] = h;
    }
}

// ---- host: the rule, exactly ------------------------------------------------------------------------------------------------
struct Queries {   // the per-query results, owned
    std::vector<uint32_t> label, n_within, n_labelled, n_same;
    std::vector<rk_hit> nearest, runner_up;
    explicit Queries(uint32_t q) : label(q, kNone), n_within(q, 0), n_labelled(q, 0), n_same(q, 0), nearest(q, absent_record()), runner_up(q, absent_record()) {}
};

inline bool present(const rk_hit &h) { return h.row != kNone; }

// x comes before the present or absent `best` of the same query: the larger ratio, then the smaller reference
inline bool nearer(const rk_hit &x, const rk_hit &best, int metric)
{
    if (!present(best)) return true;
    long long cx, ux, cb, ub;
    ratio_terms(x.common, x.size0, x.size1, metric, &cx, &ux);
    ratio_terms(best.common, best.size0, best.size1, metric, &cb, &ub);
    const __int128 l = (__int128)cx * ub, r = (__int128)cb * ux;
    return l != r ? l > r : x.col < best.col;
}

int check_labels(const uint32_t *labels, uint32_t n)
{
    for (uint32_t v = 0; v < n; v++)
        if (labels[v] >= n && labels[v] != kNone) return RK_ERR_ARG;
    return RK_OK;
}

inline bool has_counts(const rk_assign_queries *g) { return g && g->label && g->n_within && g->n_labelled && g->n_same; }

// the rule over a hit list; RK_ERR_ARG / RK_ERR_UNSUPPORTED as rk_assign_hits answers them (labels are checked by the caller)
int assign_of_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n_query, uint32_t n_ref, const uint32_t *labels, int metric, Queries *r)
{
    for (uint64_t e = 0; e < n_hits; e++)
        if (hits[e].row >= n_query || hits[e].col >= n_ref) return RK_ERR_ARG;
    for (uint64_t e = 0; e < n_hits; e++) {
        long long c, u;
        ratio_terms(hits[e].common, hits[e].size0, hits[e].size1, metric, &c, &u);
        if (!(c > 0 && c <= u)) return RK_ERR_UNSUPPORTED;
    }
    for (uint64_t e = 0; e < n_hits; e++) {   // counts, the nearest labelled reference
        const rk_hit &h = hits[e];
        r->n_within[h.row]++;
        if (labels[h.col] == kNone) continue;
        r->n_labelled[h.row]++;
        if (nearer(h, r->nearest[h.row], metric)) r->nearest[h.row] = h;
    }
    for (uint32_t q = 0; q < n_query; q++)
        if (present(r->nearest[q])) r->label[q] = labels[r->nearest[q].col];
    for (uint64_t e = 0; e < n_hits; e++) {   // the support, the runner-up
        const rk_hit &h = hits[e];
        const uint32_t l = labels[h.col];
        if (l == kNone) continue;
        if (l == r->label[h.row]) r->n_same[h.row]++;
        else if (nearer(h, r->runner_up[h.row], metric)) r->runner_up[h.row] = h;
    }
    return RK_OK;
}

// the rows of the shard of `opts` among q query rows (RowShard: blocks of row_block rows, this shard owns blocks row_first,
// row_first + row_step, ...)
struct Selected {
    RowShard rows;
    Selected(const rk_dist_opts *o, uint32_t q) : rows(o, q, 0) {}
    bool operator()(uint32_t r) const
    {
        const uint64_t blk = r / rows.row_block;
        return blk >= rows.row_first && (blk - rows.row_first) % rows.row_step == 0;
    }
};

// the entries of the selected rows, from arrays of q entries each (src.nearest / src.runner_up may be null when out's are)
void hand_over(const rk_assign_queries &src, uint32_t q, const Selected *sel, rk_assign_queries *out)
{
    for (uint32_t i = 0; i < q; i++) {
        if (sel && !(*sel)(i)) continue;
        out->label[i] = src.label[i];
        out->n_within[i] = src.n_within[i];
        out->n_labelled[i] = src.n_labelled[i];
        out->n_same[i] = src.n_same[i];
        if (out->nearest) out->nearest[i] = src.nearest[i];
        if (out->runner_up) out->runner_up[i] = src.runner_up[i];
    }
}

inline rk_assign_queries view(Queries &r)
{
    return rk_assign_queries{r.label.data(), r.n_within.data(), r.n_labelled.data(), r.n_same.data(), r.nearest.data(), r.runner_up.data()};
}

// placed, novel and ambiguous of the selected rows
void census(const rk_assign_queries &g, uint32_t q, const Selected &sel, rk_assign_stats *st)
{
    for (uint32_t i = 0; i < q; i++) {
        if (!sel(i)) continue;
        if (g.label[i] == kNone) st->novel++;
        else {
            st->placed++;
            if (g.n_labelled[i] > g.n_same[i]) st->ambiguous++;
        }
    }
}

// jorc and dist of the present records of an array with the C library's log (a record that took part lies within the exact threshold:
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

// rk_dist_rows + the host's rule, inside the call: RK_ASSIGN_DEVICE=0 (the A/B leg of tools/assign_probe.py) and joins beyond 31 bits
int host_leg(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts, const uint32_t *labels, const Selected &sel,
             rk_assign_queries *out, rk_assign_stats *st)
{
    const uint32_t Q = queries->n, N = idx->n_ref;
    rk_hit *hits = nullptr;
    uint64_t n_hits = 0;
    if (int rc = rk_dist_rows(ctx, idx, queries, opts, &hits, &n_hits, nullptr)) return rc;
    Queries r(Q);
    const int rc = assign_of_hits(hits, n_hits, Q, N, labels, opts->metric != 0, &r);
    rk_free_host(hits);
    if (rc == RK_ERR_ARG) return rk_fail(ctx, RK_ERR_HIP, "rk_assign_rows: hit records name a query or a reference beyond their number");
    if (rc)
        return rk_fail(ctx, rc, "rk_assign_rows: hit records lie outside 0 < common <= u (sketches that repeat hashes): they have no place in the order");
    const rk_assign_queries g = view(r);
    hand_over(g, Q, &sel, out);
    st->edges = n_hits;
    census(g, Q, sel, st);
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_assign_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n_query, uint32_t n_ref, const uint32_t *labels, int metric, rk_assign_queries *out)
{
    if (!out || (n_hits && !hits) || (n_ref && !labels) || (n_query && !has_counts(out))) return RK_ERR_ARG;
    if (int rc = check_labels(labels, n_ref)) return rc;
    Queries r(n_query);
    if (int rc = assign_of_hits(hits, n_hits, n_query, n_ref, labels, metric != 0, &r)) return rc;
    hand_over(view(r), n_query, nullptr, out);
    return RK_OK;
}

int rk_assign_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts, const uint32_t *labels, rk_assign_queries *out,
                   rk_assign_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_assign_stats st;
    memset(&st, 0, sizeof st);
    const char *const who = "rk_assign_rows";
    if (!queries) return rk_fail(ctx, RK_ERR_ARG, "%s places explicit queries: queries is null", who);
    const uint32_t N = idx->n_ref, Q = queries->n;
    if (!out) return rk_fail(ctx, RK_ERR_ARG, "%s: out is null", who);
    if (N && !labels) return rk_fail(ctx, RK_ERR_ARG, "%s: labels is null", who);
    if (Q && !has_counts(out)) return rk_fail(ctx, RK_ERR_ARG, "%s: label, n_within, n_labelled or n_same of out is null", who);
    if (opts->triangle != 0) return rk_fail(ctx, RK_ERR_ARG, "%s works on a query join: triangle must be 0", who);
    if (rk_dense_mode(opts))
        return rk_fail(ctx, RK_ERR_ARG, "%s: a dense report (a threshold of 1.0 or above) is not offered: pairs that share nothing carry no order", who);
    if (opts->kmer_size <= 0) return rk_fail(ctx, RK_ERR_ARG, "kmer_size must be positive");
    if (opts->row_block < 0) return rk_fail(ctx, RK_ERR_ARG, "row_block must be >= 0");
    if (!Q) {
        if (stats) *stats = st;
        return RK_OK;
    }
    if (check_labels(labels, N)) return rk_fail(ctx, RK_ERR_ARG, "%s: a label is neither below the number of references nor RK_ASSIGN_NONE", who);
    const Selected sel(opts, Q);
    if (!N) {   // no join: every selected query is novel
        Queries r(Q);
        const rk_assign_queries g = view(r);
        hand_over(g, Q, &sel, out);
        census(g, Q, sel, &st);
        if (stats) *stats = st;
        return RK_OK;
    }
    if (queries->wide != idx->wide) return rk_fail(ctx, RK_ERR_ARG, "query sketches and index use different hash widths");
    if (!idx->d_postings || !idx->d_upos || idx->n_shards > 1)
        return rk_fail(ctx, RK_ERR_ARG, "%s: an index without posting lists (rk_index_join_shard, a shard of a sharded build) answers no explicit queries", who);
    if (idx->max_ref_size >= (1ULL << 30) || queries->max_size >= (1ULL << 30))
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: a sketch of 2^30 hashes or more is beyond the 62-bit ratio key", who);
    const TimedSpan span{ctx, RK_MS_ASSIGN};
    span.clear();
    const bool records = out->nearest || out->runner_up;

    if (rk_switched_off("RK_ASSIGN_DEVICE")) {
        if (int rc = host_leg(ctx, idx, queries, opts, labels, sel, out, &st)) return rc;
        if (stats) *stats = st;
        return RK_OK;
    }

    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    int rc = RK_OK;
    {
        EdgeStage stage(ctx, idx, opts, who, kPassGreedyKeys, Tail::bytes(Q, records), queries);   // with slot numbers; the tail: the results
        stage.tail_in_pass = false;   // (the key pass writes none of them)
        DevBuf<unsigned long long> w(ctx), rc_(ctx), best_w(ctx), second_w(ctx);
        DevBuf<uint32_t> dlabels(ctx), best_nb(ctx), second_nb(ctx);
        RK_HIP(ctx, dlabels.alloc(N));
        RK_HIP(ctx, best_w.alloc(Q));
        RK_HIP(ctx, second_w.alloc(Q));
        RK_HIP(ctx, best_nb.alloc(Q));
        RK_HIP(ctx, second_nb.alloc(Q));
        // the labels, once (pageable memory of the caller: the stage's first read-back synchronises the stream before this call returns)
        RK_HIP(ctx, hipMemcpyAsync(dlabels.p, labels, (size_t)N * 4, hipMemcpyHostToDevice, stream));

        // the key pass: nothing is counted before the stage is through
        rc = stage.run([&](int pass) { return query_key_pass(stage, pass, w, rc_); });
        if (!stage.beyond_31_bits(rc)) {
            if (rc) return rc;
            stage.stats(&st);
            // the borderline records, decided before any count
            if ((rc = stage.revive(w.p, &st.borderline_kept))) return rc;
            const unsigned long long n_rec = stage.n_hits;
            const unsigned grid = grid_for(ctx, n_rec), qgrid = grid_for(ctx, Q);
            const Tail dev(stage.tail(), Q);
            rk_hit *const no_records = nullptr;
            RK_HIP(ctx, hipMemsetAsync(dev.n_within, 0, (size_t)Q * 12, stream));   // the three counts
            hipLaunchKernelGGL(k_assign_init, dim3(qgrid), dim3(kStageThreads), 0, stream, best_w.p, second_w.p, best_nb.p, second_nb.p, records ? dev.nearest : no_records,
                               records ? dev.runner_up : no_records, Q);
            RK_HIP(ctx, hipGetLastError());
            RK_HIP(ctx, span.begin());
            const bool combine = !rk_switched_off("RK_ASSIGN_COMBINE");
            const auto first = combine ? k_assign_first<true> : k_assign_first<false>;
            const auto second = combine ? k_assign_second<true> : k_assign_second<false>;
            const auto settle1 = combine ? k_assign_settle<false, true> : k_assign_settle<false, false>;
            const auto settle2 = combine ? k_assign_settle<true, true> : k_assign_settle<true, false>;
            hipLaunchKernelGGL(first, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, dlabels.p, dev.n_within, dev.n_labelled, best_w.p);
            hipLaunchKernelGGL(settle1, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, dlabels.p, dev.label, best_w.p, best_nb.p);
            hipLaunchKernelGGL(k_assign_label, dim3(qgrid), dim3(kStageThreads), 0, stream, dlabels.p, best_nb.p, dev.label, Q);
            hipLaunchKernelGGL(second, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, dlabels.p, dev.label, dev.n_same, second_w.p, (int)records);
            st.sweeps = 3;
            if (records) {
                hipLaunchKernelGGL(settle2, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, dlabels.p, dev.label, second_w.p, second_nb.p);
                hipLaunchKernelGGL(k_assign_gather, dim3(grid), dim3(kStageThreads), 0, stream, stage.hits.p, w.p, rc_.p, n_rec, best_nb.p, second_nb.p, dev.nearest,
                                   dev.runner_up);
                st.sweeps = 5;
            }
            RK_HIP(ctx, hipGetLastError());
            RK_HIP(ctx, span.end());
            if ((rc = stage.fetch_home())) return rc;
            span.read();
            // nothing of the caller's is written before every check is through
            const Tail home((void *)stage.home_tail(), Q);
            unsigned long long within_sum = 0;
            for (uint32_t q = 0; q < Q; q++) {
                within_sum += home.n_within[q];
                const bool placed = home.label[q] != kNone;
                bool ok = home.n_labelled[q] <= home.n_within[q] && home.n_same[q] <= home.n_labelled[q] && placed == (home.n_labelled[q] != 0) &&
                          placed == (home.n_same[q] != 0) && (sel(q) || !home.n_within[q]) && (!placed || home.label[q] < N);
                if (ok && records) {
                    const rk_hit &a = home.nearest[q], &b = home.runner_up[q];
                    ok = present(a) == placed && present(b) == (home.n_labelled[q] > home.n_same[q]) &&
                         (!present(a) || (a.row == q && a.col < N && labels[a.col] == home.label[q])) &&
                         (!present(b) || (b.row == q && b.col < N && labels[b.col] != home.label[q] && labels[b.col] != kNone));
                }
                if (!ok) return rk_fail(ctx, RK_ERR_HIP, "%s: the counts and records of query %u do not match each other (internal error)", who, q);
            }
            const unsigned long long live = n_rec - stage.n_border + st.borderline_kept;
            if (within_sum != live) return rk_fail(ctx, RK_ERR_HIP, "%s: the counts of %u queries do not add up to the records (internal error)", who, Q);
            const rk_assign_queries g{home.label, home.n_within, home.n_labelled, home.n_same, records ? home.nearest : nullptr, records ? home.runner_up : nullptr};
            census(g, Q, sel, &st);
            if ((uint64_t)st.placed + st.novel != sel.rows.n_rows())
                return rk_fail(ctx, RK_ERR_HIP, "%s: placed and novel queries do not add up to the selected rows (internal error)", who);
            if (records && (!exact_values(home.nearest, Q, opts) || !exact_values(home.runner_up, Q, opts)))
                return rk_fail(ctx, RK_ERR_HIP, "%s: a record lies beyond the exact threshold (internal error)", who);
            hand_over(g, Q, &sel, out);
            if (stats) *stats = st;
            return RK_OK;
        }
    }
    // more records than 31-bit record numbers hold (every device buffer above has gone back to the pool): the host's rule
    memset(&st, 0, sizeof st);
    if ((rc = host_leg(ctx, idx, queries, opts, labels, sel, out, &st))) return rc;
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
