// rk_edge_stage.h -- the first stage of rk_cluster.hip, rk_forest.hip, rk_greedy.hip, rk_knn.hip, rk_dbscan.hip, rk_mreach.hip,
// rk_medoid.hip and -- over a QUERY join: EdgeStage::queries, with a key pass of its own -- rk_assign.hip (not part of the public ABI): the self join into a device buffer and one pass over its records that tells the BORDERLINE ones from those the device
// may decide.  DESIGN.md 4.6.  The key pass of all but the first lives here too (k_edge_keys, EdgeStage::key_pass); rk_cluster.hip brings
// its own.  Two passes over the keyed records that more than one caller runs behind the stage follow it: k_edge_revive (greedy,
// dbscan, mreach, medoid) and k_edge_degree (knn, dbscan, mreach).  So does the host code that every caller would otherwise repeat
// around the stage: the refusals in front of it (StageNeeds, stage_options, stage_index), EdgeStage::revive (decide, the kept slot
// numbers back up, k_edge_revive), EdgeStage::beyond_31_bits (the way to a caller's host leg) and EdgeStage::stats; the timed span
// around a caller's kernels is TimedSpan of rk_internal.h.
//
//   join     rk_dist_rows_dev with the threshold widened by 2^-46 (capped at 1.0: beyond it the public join would turn to the dense
//            report) appends unordered hit records to a buffer of max(65,536, rows * 64) records; its counter counts every hit,
//            those beyond the capacity included;
//   pass     the caller's kernel over the records that were written.  A record whose device distance is not below D (1 - 2^-46)
//            is BORDERLINE (the device's log may differ from the C library's in the last bits): edge_append sends what rk_distance
//            needs of it to a small buffer (4,096 records, RK_CLUSTER_EDGE_CAP), the device leaves it alone;
//   retries  more hits than the buffer holds: the join again with the exact count, every counter reset; more borderline records than
//            theirs holds: the pass alone again, the borderline counter reset.  Each at most once;
//   decide   the borderline records come home and rk_host_exact_distances (the C library's log, the reference's strict `<` of
//            src/dist.cpp:232; the non-strict `<=` of :624 for a query join) keeps or drops each.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_edge_order.h"

namespace {

constexpr uint32_t kStageThreads = 256;      // threads of the first pass and of the passes that follow it
constexpr uint64_t kEdgeCapDefault = 4096;   // borderline records the first pass has room for (RK_CLUSTER_EDGE_CAP)

// the counters of the stage, in front of the caller's tail (u64 each)
enum { kCntHits = 0, kCntBorder = 1, kCntBad = 2, kCntRange = 3, kCntWords = 4 };

struct rk_edge {   // a borderline record: what rk_distance needs
    uint32_t row, col;
    int32_t common, size0, size1;
};

inline unsigned grid_for(const rk_ctx *ctx, uint64_t items)
{
    const uint64_t want = (items + kStageThreads - 1) / kStageThreads;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)std::max(1, ctx->num_cu) * 8));
}

// n records for the caller of the library (rk_free_host): never a null pointer for an empty result
inline rk_hit *host_records(uint64_t n)
{
    return (rk_hit *)malloc((n ? n : 1) * sizeof(rk_hit));
}

// The adjacency of a hit list over n genomes (the caller has checked row, col < n): the numbers of the records incident to genome v,
// ascending, are adj[start[v] .. start[v + 1]) -- a counting sort of record numbers by endpoint.
inline void hit_adjacency(const rk_hit *hits, uint64_t n_hits, uint32_t n, std::vector<uint64_t> *start, std::vector<uint64_t> *adj)
{
    std::vector<uint64_t> &at = *start;
    at.assign((size_t)n + 2, 0);
    for (uint64_t e = 0; e < n_hits; e++) {
        at[hits[e].row + 2]++;
        at[hits[e].col + 2]++;
    }
    for (size_t i = 2; i < at.size(); i++) at[i] += at[i - 1];
    adj->resize(2 * n_hits);
    for (uint64_t e = 0; e < n_hits; e++) {   // (at[v + 1] runs from the begin of v's records to their end)
        (*adj)[at[hits[e].row + 1]++] = e;
        (*adj)[at[hits[e].col + 1]++] = e;
    }
    at.pop_back();
}

// record e is borderline: counted always, stored while there is room (the host sees the overflow from the counter)
__device__ __forceinline__ void edge_append(const rk_hit &h, unsigned long long e, rk_edge *edges, unsigned long long *slots, unsigned long long edge_cap,
                                            unsigned long long *n_border)
{
    const unsigned long long at = atomicAdd(n_border, 1ULL);
    if (at < edge_cap) {
        edges[at] = rk_edge{h.row, h.col, h.common, h.size0, h.size1};
        if (slots) slots[at] = e;
    }
}

// The first pass of the forest and of the greedy rule: per record w (rk_edge_order.h) and row << 32 | col.  A borderline record is
// dead on the device (for now).  A record outside 0 < common <= u (multisets) has no key: the forest sends it to the host with the
// borderline ones; GREEDY counts it (the representatives cannot be patched afterwards: the call refuses the collection) and stores
// the slot number of every borderline record, so that the ones the host keeps can be revived.
// cnt[kCntHits] counts every hit of the join, those beyond `cap` included: the pass reads what was written.
template <bool GREEDY>
__global__ void __launch_bounds__(kStageThreads)
k_edge_keys(const rk_hit *hits, unsigned long long *cnt, unsigned long long cap, uint32_t n, double link_below, int metric, unsigned long long *w_out,
            unsigned long long *rc_out, rk_edge *edges, unsigned long long *slots, unsigned long long edge_cap)
{
    const unsigned long long n_rec = min(cnt[kCntHits], cap);
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const rk_hit h = hits[e];
        rc_out[e] = ((unsigned long long)h.row << 32) | h.col;
        long long c, u;
        ratio_terms(h.common, h.size0, h.size1, metric, &c, &u);
        const bool bad = h.row >= n || h.col >= n || h.row == h.col;   // (never from the join's kernels; nothing is indexed by such a record)
        const bool keyed = c > 0 && c <= u;
        unsigned long long w = kDead;
        if (bad || (GREEDY && !keyed)) atomicAdd(cnt + (bad ? kCntBad : kCntRange), 1ULL);
        else if (!keyed || !(h.dist < link_below)) edge_append(h, e, edges, GREEDY ? slots : nullptr, edge_cap, cnt + kCntBorder);
        else w = ~ratio_key((unsigned long long)c, (unsigned long long)u);   // (key >= 1: never kDead)
        w_out[e] = w;
    }
}

// the borderline records the host kept (their slot numbers, sent back up): alive from here on, their keys from the same integer
// function.  (maybe_unused, here and below: not every file that includes the stage runs these two)
[[maybe_unused]] __global__ void k_edge_revive(const rk_hit *hits, const unsigned long long *slots, unsigned long long n_kept, unsigned long long n_rec, int metric,
                              unsigned long long *w)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_kept) return;
    const unsigned long long e = slots[i];
    if (e >= n_rec) return;   // (the host sends back what k_edge_keys wrote)
    const rk_hit h = hits[e];
    long long c, u;
    ratio_terms(h.common, h.size0, h.size1, metric, &c, &u);
    w[e] = ~ratio_key((unsigned long long)c, (unsigned long long)u);   // (k_edge_keys saw 0 < c <= u)
}

// deg[v] += the live records incident to v.  Behind the stage, never inside its pass: the pass may run twice
[[maybe_unused]] __global__ void __launch_bounds__(kStageThreads)
k_edge_degree(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, uint32_t *deg)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        if (w[e] == kDead) continue;
        const unsigned long long p = rc[e];
        atomicAdd(deg + (uint32_t)(p >> 32), 1u);
        atomicAdd(deg + (uint32_t)p, 1u);
    }
}

// What a call asks in front of the stage, beyond a self join.  The refusals come in two halves, in this order, with the caller's
// `if (!N) return RK_OK` and whatever it checks itself between them: stage_options (triangle, row shard, dense report), stage_index
// (rk_self_join_args, join-only index, ratio key).
struct StageNeeds {
    const char *who;         // the call's name
    const char *every_row;   // why the call does not compose from row shards (null: it does).  Such a call has no use for a join-only index either: that holds the rows of one shard
    bool ratio_key;          // the call orders records by ratio_key: no dense report, no sketch of 2^30 hashes (all but rk_cluster_rows)
};

inline int stage_options(rk_ctx *ctx, const StageNeeds &needs, const rk_dist_opts *opts)
{
    if (opts->triangle != 1) return rk_fail(ctx, RK_ERR_ARG, "%s works on a self join: triangle must be 1", needs.who);
    if (needs.every_row && opts->row_step > 1) return rk_fail(ctx, RK_ERR_ARG, "%s needs every row: %s", needs.who, needs.every_row);
    if (needs.ratio_key && rk_dense_mode(opts))
        return rk_fail(ctx, RK_ERR_ARG, "%s: a dense report (a threshold above 1.0) is not offered: pairs that share nothing carry no order", needs.who);
    return RK_OK;
}

inline int stage_index(rk_ctx *ctx, const StageNeeds &needs, const rk_index *idx, const rk_dist_opts *opts)
{
    if (int rc = rk_self_join_args(ctx, idx, opts)) return rc;
    if (needs.every_row && !idx->d_postings) return rk_fail(ctx, RK_ERR_ARG, "%s: a join-only index (rk_index_join_shard) holds the rows of one shard", needs.who);
    if (needs.ratio_key && idx->max_ref_size >= (1ULL << 30))
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: a sketch of 2^30 hashes or more is beyond the 62-bit ratio key", needs.who);
    return RK_OK;
}

// the first pass a stage will run: the caller's own, key_pass<false>, or key_pass<true> (with the slot numbers of the borderline records)
enum StagePass { kPassOwn, kPassKeys, kPassGreedyKeys };

struct EdgeStage {
    rk_ctx *ctx;
    const rk_index *idx;
    const rk_sketches *queries;  // null: the self join (all callers but rk_assign_rows); else the rows are these queries
    uint32_t n_rows;             // rows of the join: genomes of the index, or queries
    const rk_dist_opts *exact;   // the caller's options: the threshold the host decides with
    const char *who;             // the caller's name, for the texts that carry it
    const char *hits_what;       // what a capacity's worth of device memory holds, for the text of its refusal
    const char *bad_what;        // what the pass counts in kCntBad
    rk_dist_opts widened;        // the join reports with the widened threshold,
    double link_below;           // the device decides what lies below the narrowed one, the host the rest
    int metric;
    uint64_t cap, edge_cap;
    DevBuf<rk_hit> hits;         // lives as long as the stage: later passes of the caller read it here
    DevBuf<rk_edge> edges;
    DevBuf<unsigned long long> slots, block;   // slots: with_slots only.  block: the counters, then the caller's tail
    size_t tail_bytes;
    bool with_slots;                           // kPassGreedyKeys
    bool tail_in_pass = true;                  // false: the pass does not write the tail; run() brings the counters home alone and the caller's fetch_home() the tail
    const unsigned char *home = nullptr;       // counters and tail of the last pass in the context's page-locked scratch
    unsigned long long n_hits = 0, n_border = 0;
    uint32_t join_attempts = 0, pass_attempts = 0;   // (pass_attempts: those behind the last join)

    EdgeStage(rk_ctx *c, const rk_index *index, const rk_dist_opts *opts, const char *name, StagePass pass, size_t tail = 0, const rk_sketches *qs = nullptr)
        : ctx(c), idx(index), queries(qs), n_rows(qs ? qs->n : index->n_ref), exact(opts), who(name),
          hits_what(pass == kPassOwn ? "hit records" : "hit records and their keys"),
          bad_what(qs ? "a query or a reference beyond their number" : pass == kPassGreedyKeys ? "a genome beyond the index or one genome twice" : "a genome beyond the index"),
          widened(*opts), link_below(opts->max_dist), metric(opts->metric != 0),
          cap(rk_hit_capacity(RowShard(opts, n_rows, n_rows).n_rows())),   // (the rows of this shard, as rk_dist_rows counts them)
          edge_cap(kEdgeCapDefault), hits(c), edges(c), slots(c), block(c), tail_bytes(tail), with_slots(pass == kPassGreedyKeys)
    {
        if (opts->max_dist > 0.0) {
            // (a query join turns dense AT 1.0, the self join beyond it: rk_dense_mode)
            widened.max_dist = std::min(opts->max_dist + opts->max_dist * kBorderRel, qs ? std::nextafter(1.0, 0.0) : 1.0);
            link_below = opts->max_dist - opts->max_dist * kBorderRel;
        }
        if (const char *e = getenv("RK_CLUSTER_EDGE_CAP")) edge_cap = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    }
    unsigned long long *cnt() const { return block.p; }
    void *tail() const { return block.p + kCntWords; }
    const unsigned char *home_tail() const { return home + kCntWords * 8; }

    int alloc_edges()
    {
        RK_HIP(ctx, edges.alloc(edge_cap));
        if (with_slots) RK_HIP(ctx, slots.alloc(edge_cap));
        return RK_OK;
    }

    // pass(k): the caller enqueues its k-th pass (k = 0, 1) over hits.p behind a join, on ctx->stream; buffers of `cap` records are
    // its own, allocated at k = 0.  The pass may have side effects that hold whatever follows (rk_cluster_rows links while it
    // classifies: a link made once is a link of the result).  Counters and tail come home in one copy, one synchronisation.
    template <class Pass> int run(Pass &&pass)
    {
        hipStream_t stream = ctx->stream;
        const size_t block_bytes = kCntWords * 8 + tail_bytes;
        RK_HIP(ctx, block.alloc((block_bytes + 7) / 8));
        if (int rc = alloc_edges()) return rc;
        for (int attempt = 0; attempt < 2; attempt++) {
            if (hits.alloc(cap) != hipSuccess) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu %s on the device", (unsigned long long)cap, hits_what);
            RK_HIP(ctx, hipMemsetAsync(block.p, 0, kCntWords * 8, stream));
            if (int rc = rk_dist_rows_dev(ctx, idx, queries, &widened, hits.p, cap, (uint64_t *)(block.p + kCntHits), stream)) return rc;
            join_attempts++;
            pass_attempts = 0;
            for (int k = 0; k < 2; k++) {
                if (int rc = pass(k)) return rc;
                if (int rc = fetch_home(tail_in_pass)) return rc;   // (the scratch is asked for behind the join, whose lazy builders use it too)
                unsigned long long c[kCntWords];
                memcpy(c, home, sizeof c);
                if (c[kCntBad]) return rk_fail(ctx, RK_ERR_HIP, "%llu hit records name %s", c[kCntBad], bad_what);
                n_hits = c[kCntHits];
                n_border = c[kCntBorder];
                if (n_hits > cap) break;   // overflow: the join again with the exact count
                if (c[kCntRange])
                    return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: %llu hit records lie outside 0 < common <= u (sketches that repeat hashes): they have no place in the order",
                                   who, c[kCntRange]);
                pass_attempts++;
                if (n_border <= edge_cap) return RK_OK;
                edge_cap = n_border;   // the pass alone again, with room for every borderline record
                if (int rc = alloc_edges()) return rc;
                RK_HIP(ctx, hipMemsetAsync(block.p + kCntBorder, 0, 8, stream));
            }
            if (n_hits <= cap) break;
            cap = n_hits;
        }
        return rk_fail(ctx, RK_ERR_CAPACITY, "hit or borderline buffer overflow persisted after resize");
    }

    // counters and (with_tail) tail of the block into the context's page-locked scratch: one copy, one synchronisation
    int fetch_home(bool with_tail = true)
    {
        const size_t bytes = kCntWords * 8 + (with_tail ? tail_bytes : 0);
        home = (const unsigned char *)rk_pinned_scratch(ctx, bytes);
        if (!home) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %zu bytes of page-locked memory for the labels", bytes);
        RK_HIP(ctx, hipMemcpyAsync((void *)home, block.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        RK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return RK_OK;
    }

    // The key pass of the forest, the greedy rule, the neighbour lists and the density clusters as pass k of run(): k_edge_keys<GREEDY> over w and rc of
    // `cap` records each.  The buffers are the caller's (its later passes read them), allocated here at k = 0, and `extra` (greedy's
    // hl) with them where one is given.
    template <bool GREEDY>
    int key_pass(int k, DevBuf<unsigned long long> &w, DevBuf<unsigned long long> &rc, DevBuf<unsigned long long> *extra = nullptr)
    {
        if (!k && (w.alloc(cap) != hipSuccess || rc.alloc(cap) != hipSuccess || (extra && extra->alloc(cap) != hipSuccess)))
            return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu %s on the device", (unsigned long long)cap, hits_what);
        hipLaunchKernelGGL(k_edge_keys<GREEDY>, dim3(grid_for(ctx, cap)), dim3(kStageThreads), 0, ctx->stream, hits.p, cnt(), (unsigned long long)cap,
                           idx->n_ref, link_below, metric, w.p, rc.p, edges.p, GREEDY ? slots.p : (unsigned long long *)nullptr,
                           (unsigned long long)edge_cap);
        RK_HIP(ctx, hipGetLastError());
        return RK_OK;
    }

    // The borderline records, decided: the ones the exact threshold keeps, in the order the pass stored them, with the C library's
    // jorc and dist; kept_slots (with_slots): the slot numbers of those.
    int decide(std::vector<rk_hit> *kept, std::vector<unsigned long long> *kept_slots = nullptr)
    {
        kept->clear();
        if (!n_border) return RK_OK;
        hipStream_t stream = ctx->stream;
        std::vector<rk_edge> e(n_border);
        std::vector<unsigned long long> slot(kept_slots ? n_border : 0);
        RK_HIP(ctx, hipMemcpyAsync(e.data(), edges.p, n_border * sizeof(rk_edge), hipMemcpyDeviceToHost, stream));
        if (kept_slots) RK_HIP(ctx, hipMemcpyAsync(slot.data(), slots.p, n_border * 8, hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipStreamSynchronize(stream));
        kept->resize(n_border);
        for (size_t i = 0; i < e.size(); i++)   // (pad_, where slots are asked for: the record's place in `slot`)
            (*kept)[i] = rk_hit{e[i].row, e[i].col, e[i].common, e[i].size0, e[i].size1, kept_slots ? (int32_t)i : 0, 0.0, 0.0};
        kept->resize(rk_host_exact_distances(kept->data(), n_border, exact));
        if (kept_slots) {
            kept_slots->resize(kept->size());
            for (size_t i = 0; i < kept->size(); i++) (*kept_slots)[i] = slot[(size_t)(*kept)[i].pad_];
        }
        return RK_OK;
    }

    // decide() for the callers that stage with slot numbers, before their first pass behind the stage: the slot numbers of the records
    // the host kept go back up and k_edge_revive makes those alive in w (the caller's keys); nothing is copied or launched when none is
    // kept.  *n_kept: how many were.
    int revive(unsigned long long *w, uint64_t *n_kept)
    {
        // (never in rk_mreach_rows, which goes to the host from 2^31 hits on: n_border <= n_hits)
        if (n_border >= (1ULL << 31)) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: %llu borderline records", who, n_border);
        std::vector<rk_hit> kept;
        std::vector<unsigned long long> kept_slots;
        if (int rc = decide(&kept, &kept_slots)) return rc;
        *n_kept = kept.size();
        if (kept.empty()) return RK_OK;
        RK_HIP(ctx, hipMemcpyAsync(slots.p, kept_slots.data(), kept_slots.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        RK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (kept_slots is pageable memory)
        hipLaunchKernelGGL(k_edge_revive, dim3((unsigned)((kept.size() + kStageThreads - 1) / kStageThreads)), dim3(kStageThreads), 0, ctx->stream, hits.p,
                           slots.p, (unsigned long long)kept.size(), n_hits, metric, w);
        RK_HIP(ctx, hipGetLastError());
        return RK_OK;
    }

    // run() returned rc with more records than 31-bit record numbers hold, or without the memory for that many: the hit buffer goes
    // back to the pool, the caller releases its own buffers and takes its host leg
    bool beyond_31_bits(int rc)
    {
        if ((rc && rc != RK_ERR_NOMEM) || n_hits < (1ULL << 31)) return false;
        hits.reset();
        return true;
    }

    // what every caller's stats say about the stage (rk_cluster_stats has its own name for the passes)
    template <class Stats> void stats(Stats *st) const
    {
        st->join_attempts = join_attempts;
        st->border_attempts = pass_attempts;
        st->edges = n_hits;
        st->borderline = n_border;
    }
};

}  // namespace
