// rk_topn.hip -- `dist -N` on the device (rk_dist_topn): per query row the max_neighbor nearest references, without the
// Q x R hit records of a dense report (the default -D 1.0 makes every cell a hit: rk_dist_rows would hold 40 B per cell on
// the device and on the host, src/dist.cpp:599,625-640,683-689 keeps N of them per row).
//
// Per batch of query rows (as many counter rows as RK_TOPN_BATCH_BYTES holds):
//   stage A  rk_distq_kernel in counts-only mode (rk_distq_counts): the rows' intersection counts, columns in the caller's
//            reference order, into an int32 scratch of one batch;
//   stage B  k_topn_select, one workgroup per row: walks the row in column order and emits the cells that may matter to the
//            reference's heap -- a superset of (the first N cells of the stream) + (every cell that beats the heap top at its
//            arrival) -- as candidate records;
//   host     candidates ordered by (row, col) (device radix sort), downloaded, recomputed with the C library's log and the
//            exact threshold (rk_host_exact_distances), replayed through the reference's heap (rk_topn_rows).
// Why replaying a superset of that kind gives the reference's heap bit for bit, and the margins that keep stage B's set a
// superset: DESIGN.md, "dist -N on the device".
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_dist_common.h"

namespace {

constexpr uint32_t kTopnMaxN = 1024;      // largest max_neighbor the selection kernel holds in LDS (beyond: rk_dist_rows + rk_topn_rows)
constexpr uint32_t kSelThreads = 256;
constexpr uint32_t kSelPer = 4;            // cells per thread and step once N certain cells are known (one before)
constexpr uint32_t kBestCap = kTopnMaxN + kSelThreads * kSelPer;   // best N + one step's additions
constexpr double kDistMargin = 0x1p-40;    // relative: device log vs the C library's (a few ulps) -- far inside
constexpr double kJorcMargin = 0x1p-20;    // relative, on jaccard/containment bounds derived through exp()

struct SelArgs {
    const int32_t *counts;      // [n_slots][n_ref], caller column order (stage A)
    const uint32_t *sizes;      // u32[n_ref] reference sketch sizes, caller order
    const uint64_t *q_off;      // u64[n_query + 1]
    uint32_t n_ref, n_query, slot_base, row_first, row_step, row_block;
    uint32_t max_n;
    int32_t metric, kmer_size;
    double max_dist;            // the EXACT -D
    double lo_jorc;             // a cell with 0 < jorc < lo_jorc is certainly beyond max_dist
    rk_hit *cand;               // candidate records (jorc / dist left 0: the host computes them)
    unsigned long long *keys;   // row << 32 | col per candidate (the radix sort's keys)
    unsigned long long cap;
    unsigned long long *n_cand; // counts every candidate, including those beyond cap
};

// jorc below which the distance certainly exceeds d: the threshold jaccard t / (2 - t) (containment t), t = exp(-k d), shrunk
// by kJorcMargin.  0 disables the bound (d so large that t underflows; every positive jorc is at least 2^-33 anyway).
__host__ __device__ inline double jorc_below(double d, int metric, int kmer_size)
{
    const double t = exp(-(double)kmer_size * d);
    const double j = metric ? t : t / (2.0 - t);
    return j * (1.0 - kJorcMargin);
}

// One workgroup per row of the batch.  LDS: the smallest N upper distance bounds of certainly-in-stream cells seen so far
// (ascending) + the additions of the current step; after each step they are merged by a bitonic sort.  The heap top at any
// later cell is at most T = the N-th of them.  A cell is emitted when it may be in the stream (its lower bound <= -D) and
// either fewer than N certain cells came before its step or its lower bound is below T.
__global__ __launch_bounds__(kSelThreads) void k_topn_select(SelArgs a)
{
    __shared__ double best[kBestCap];
    __shared__ uint32_t s_nb, s_m;
    __shared__ double s_top, s_jt;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t local = blockIdx.x, slot = a.slot_base + local;
    const uint64_t row64 = ((uint64_t)a.row_first + (uint64_t)(slot / a.row_block) * a.row_step) * a.row_block + slot % a.row_block;
    if (row64 >= a.n_query) return;   // (uniform)
    const uint32_t row = (uint32_t)row64;
    const int qsize = (int)(a.q_off[row + 1] - a.q_off[row]);
    const int32_t *cnt = a.counts + (size_t)local * a.n_ref;
    const unsigned long long lt_mask = lane ? (~0ULL >> (64 - lane)) : 0ULL;
    if (tid == 0) {
        s_nb = 0;
        s_m = 0;
        s_top = INFINITY;
        s_jt = 0.0;
    }
    __syncthreads();
    for (uint32_t c0 = 0; c0 < a.n_ref;) {
        const uint32_t nb = s_nb;
        const bool full = nb >= a.max_n;
        const double top = s_top, jt = s_jt;
        const uint32_t per = full ? kSelPer : 1u;
        for (uint32_t i = 0; i < per; i++) {
            const uint32_t col = c0 + i * kSelThreads + tid;
            bool emit = false;
            int common = 0, size0 = 0;
            if (col < a.n_ref) {
                common = cnt[col];
                size0 = (int)a.sizes[col];   // triangle 0: size0 = |ref|, size1 = |query| (src/dist.cpp:607-608)
                const int size1 = qsize;
                double dl, du;
                bool live = true;
                if (common == 0 || size0 == 0 || size1 == 0) {   // jorc 0.0: distance exactly 1.0 (src/dist.cpp:617-618)
                    dl = du = 1.0;
                } else {
                    const double denom = a.metric ? (double)min(size0, size1) : (double)(size0 + size1 - common);
                    // key-space rejects, no log: beyond -D, or certainly not below the heap top's bound
                    if ((double)common < a.lo_jorc * denom || (full && (double)common < jt * denom)) live = false;
                    dl = du = 0.0;
                    if (live) {
                        const JorcDist jd = rk_distance(common, size0, size1, a.metric, a.kmer_size);
                        const double m = fabs(jd.dist) * kDistMargin;
                        dl = jd.dist - m;
                        du = jd.dist + m;
                    }
                }
                if (live) {
                    emit = dl <= a.max_dist && (!full || dl < top);
                    if (du <= a.max_dist && (!full || du < top)) best[nb + atomicAdd(&s_m, 1u)] = du;
                }
            }
            // per-wave append: one device-scope atomic per wave and cell slot
            const unsigned long long mask = __ballot(emit);
            if (mask) {   // (uniform in the wave)
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(a.n_cand, (unsigned long long)__popcll(mask));
                base = __shfl(base, 0);
                if (emit) {
                    const unsigned long long at = base + (unsigned long long)__popcll(mask & lt_mask);
                    if (at < a.cap) {
                        rk_hit h;
                        h.row = row;
                        h.col = col;
                        h.common = common;
                        h.size0 = size0;
                        h.size1 = qsize;
                        h.pad_ = 0;
                        h.jorc = 0.0;
                        h.dist = 0.0;
                        a.cand[at] = h;
                        a.keys[at] = ((unsigned long long)row << 32) | col;
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t m = s_m;
        __syncthreads();   // (every thread holds m before it is reset below)
        if (m) {   // (uniform) merge: bitonic sort of best[0 .. P), P the power of two at or above nb + m
            uint32_t P = 1;
            while (P < nb + m) P <<= 1;
            for (uint32_t i = nb + m + tid; i < P; i += kSelThreads) best[i] = INFINITY;
            __syncthreads();
            for (uint32_t k = 2; k <= P; k <<= 1)
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t i = tid; i < P; i += kSelThreads) {
                        const uint32_t ixj = i ^ j;
                        if (ixj > i) {
                            const double x = best[i], y = best[ixj];
                            if ((x > y) == ((i & k) == 0)) {
                                best[i] = y;
                                best[ixj] = x;
                            }
                        }
                    }
                    __syncthreads();
                }
            if (tid == 0) {
                const uint32_t nb2 = min(a.max_n, nb + m);
                s_nb = nb2;
                s_m = 0;
                if (nb2 >= a.max_n) {
                    s_top = best[a.max_n - 1];
                    s_jt = jorc_below(s_top, a.metric, a.kmer_size);
                }
            }
            __syncthreads();
        }
        c0 += per * kSelThreads;
    }
}

// reference sizes in the caller's order (the index keeps them in its internal order)
__global__ void k_sizes_caller(const uint32_t *sizes, const uint32_t *orig, uint32_t n, uint32_t *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[orig ? orig[i] : i] = sizes[i];
}

}  // namespace

extern "C" int rk_dist_topn(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts,
                            uint64_t max_neighbor, rk_hit **hits_out, uint64_t *n_hits)
{
    if (!ctx || !idx || !queries || !opts || !hits_out || !n_hits) return RK_ERR_ARG;
    *hits_out = nullptr;
    *n_hits = 0;
    if (opts->triangle) return rk_fail(ctx, RK_ERR_ARG, "-N needs explicit queries (triangle = 0): alldist has no -N");
    if (max_neighbor == 0) {   // rk_topn_rows keeps nothing either
        *hits_out = (rk_hit *)malloc(sizeof(rk_hit));
        return *hits_out ? RK_OK : rk_fail(ctx, RK_ERR_NOMEM, "host allocation failed");
    }
    RK_HIP(ctx, hipSetDevice(ctx->device));
    // sparse thresholds (the output is bounded by the hits), N beyond the LDS set, empty sides: the plain path
    if (!ctx->sw_topn || !rk_dense_mode(opts) || max_neighbor > kTopnMaxN || !idx->n_ref || !queries->n) {
        int rc = rk_dist_rows(ctx, idx, queries, opts, hits_out, n_hits, nullptr);
        if (rc) return rc;
        return rk_topn_rows(*hits_out, n_hits, max_neighbor);
    }
    if (opts->kmer_size <= 0) return rk_fail(ctx, RK_ERR_ARG, "kmer_size must be positive");
    if (opts->row_block < 0) return rk_fail(ctx, RK_ERR_ARG, "row_block must be >= 0");
    hipStream_t stream = ctx->stream;
    if (ctx->timing)
        for (int i = RK_MS_TOPN_COUNTS; i <= RK_MS_TOPN_CANDIDATES; i++) ctx->last_ms[i] = 0.0;
    // (timing on: the stages are bracketed with events on the stream -- one synchronisation more per stage)
    auto t_begin = [&]() { return ctx->timing ? hipEventRecord(ctx->ev[0], stream) : hipSuccess; };
    auto t_end = [&](int which) {
        if (!ctx->timing) return hipSuccess;
        float ms = 0.f;
        hipError_t e = hipEventRecord(ctx->ev[1], stream);
        if (e == hipSuccess) e = hipEventSynchronize(ctx->ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
        ctx->last_ms[which] += ms;
        return e;
    };
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    const uint32_t R = idx->n_ref, Q = queries->n;
    const uint32_t rb = opts->row_block > 0 ? (uint32_t)opts->row_block : 1u;
    const uint32_t rs = opts->row_step ? opts->row_step : 1u;
    // the shard's row slots (block-cyclic, as rk_distq_kernel deals them): rows ascend with the slot, the valid ones are a prefix
    uint64_t n_sel = 0;
    for (uint64_t blk = opts->row_first; blk * rb < Q; blk += rs) n_sel += std::min<uint64_t>(Q, (blk + 1) * rb) - blk * rb;
    std::vector<rk_hit> result;
    if (n_sel) {
        // candidate slots per row: one step of single cells until N certain cells are known, then ~N ln(R / 256) improvements
        // and the cells that tie the N-th bound (the margins let a tie through: configs[4], -N 5, 568 per row) -- and never more
        // than the row's R cells
        const uint64_t per_row = std::min<uint64_t>(R, 1024 + 16 * max_neighbor);
        // device bytes of one row of a batch, all inside RK_TOPN_BATCH_BYTES: its counter row and its candidate slots, each a
        // record + key, their sorted copy, and as much again for the radix sort's scratch
        const uint64_t row_bytes = (uint64_t)R * 4 + per_row * 3 * (sizeof(rk_hit) + sizeof(unsigned long long));
        const uint64_t rows_per_batch = std::max<uint64_t>(1, std::min<uint64_t>(n_sel, ctx->sw_topn_batch_bytes / row_bytes));
        DevBuf<int32_t> counts(ctx);
        DevBuf<uint32_t> sizes(ctx);
        DevBuf<unsigned long long> counter(ctx);
        if (counts.alloc(rows_per_batch * R) != hipSuccess || sizes.alloc(R) != hipSuccess || counter.alloc(1) != hipSuccess)
            return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu counter rows of %u columns", (unsigned long long)rows_per_batch, R);
        hipLaunchKernelGGL(k_sizes_caller, dim3((R + 255) / 256), dim3(256), 0, stream, idx->d_sizes,
                           idx->relabeled ? idx->d_orig : nullptr, R, sizes.p);
        RK_HIP(ctx, hipGetLastError());
        SelArgs a;
        a.counts = counts.p;
        a.sizes = sizes.p;
        a.q_off = queries->d_off;
        a.n_ref = R;
        a.n_query = Q;
        a.row_first = opts->row_first;
        a.row_step = rs;
        a.row_block = rb;
        a.max_n = (uint32_t)max_neighbor;
        a.metric = opts->metric != 0;   // (any non-zero isContainment is containment)
        a.kmer_size = opts->kmer_size;
        a.max_dist = opts->max_dist;
        a.lo_jorc = jorc_below(opts->max_dist, a.metric, a.kmer_size);
        a.n_cand = counter.p;
        // (an overflow grows it to the exact count, at most the batch's rows x R)
        uint64_t cap = ctx->sw_topn_cand_cap ? ctx->sw_topn_cand_cap : rows_per_batch * per_row;
        DevBuf<rk_hit> cand(ctx), ordered(ctx);
        DevBuf<unsigned long long> keys(ctx), keys_out(ctx);
        uint64_t ordered_cap = 0;
        std::vector<rk_hit> host;
        int bits = 33;
        while (bits < 64 && (1ULL << (bits - 32)) < Q) bits++;
        for (uint64_t s0 = 0; s0 < n_sel; s0 += rows_per_batch) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(rows_per_batch, n_sel - s0);
            RK_HIP(ctx, t_begin());
            int rc = rk_distq_counts(ctx, idx, queries, opts, (uint32_t)s0, nb, counts.p, stream);
            if (rc) return rc;
            RK_HIP(ctx, t_end(RK_MS_TOPN_COUNTS));
            unsigned long long n = 0;
            for (int attempt = 0; attempt < 2; attempt++) {
                if (!cand.p || attempt) {
                    if (cand.alloc(cap) != hipSuccess || keys.alloc(cap) != hipSuccess)
                        return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu candidate records", (unsigned long long)cap);
                }
                RK_HIP(ctx, hipMemsetAsync(counter.p, 0, 8, stream));
                a.slot_base = (uint32_t)s0;
                a.cand = cand.p;
                a.keys = keys.p;
                a.cap = cap;
                RK_HIP(ctx, t_begin());
                hipLaunchKernelGGL(k_topn_select, dim3(nb), dim3(kSelThreads), 0, stream, a);
                RK_HIP(ctx, hipGetLastError());
                RK_HIP(ctx, t_end(RK_MS_TOPN_SELECT));
                rc = rk_read_back(ctx, &n, counter.p, 8, stream);
                if (rc) return rc;
                if (n <= cap) break;
                cap = n;   // overflow: the counter rows are still there, stage B runs again with the exact count
            }
            if (n > cap) return rk_fail(ctx, RK_ERR_CAPACITY, "candidate buffer overflow persisted after resize");
            if (ctx->timing) ctx->last_ms[RK_MS_TOPN_CANDIDATES] += (double)n;
            const clk::time_point t_dl = clk::now();
            host.resize(n);
            const rk_hit *src = cand.p;
            bool on_device = false;
            if (n > (ctx->single_shot ? (1ULL << 18) : 2048ULL)) {   // (row, col) order on the device (as rk_dist_rows); on any failure the host sorts
                if (ordered_cap < n)   // (as big as the candidate buffer: later batches reuse it)
                    ordered_cap = keys_out.alloc(cap) == hipSuccess && ordered.alloc(cap) == hipSuccess ? cap : 0;
                if (ordered_cap >= n)
                    on_device = rk_prim_sort_hits(ctx, keys.p, keys_out.p, cand.p, ordered.p, n, (unsigned)bits, stream) == RK_OK;
                if (on_device) src = ordered.p;
                else (void)hipGetLastError();
            }
            if (n) {
                RK_HIP(ctx, hipMemcpyAsync(host.data(), src, n * sizeof(rk_hit), hipMemcpyDeviceToHost, stream));
                RK_HIP(ctx, hipStreamSynchronize(stream));
            }
            if (!on_device)
                std::sort(host.begin(), host.end(), [](const rk_hit &x, const rk_hit &y) {
                    return x.row != y.row ? x.row < y.row : x.col < y.col;
                });
            const clk::time_point t_host = clk::now();
            if (ctx->timing) ctx->last_ms[RK_MS_TOPN_DOWNLOAD] += std::chrono::duration<double, std::milli>(t_host - t_dl).count();
            uint64_t k = rk_host_exact_distances(host.data(), n, opts);
            rc = rk_topn_rows(host.data(), &k, max_neighbor);
            if (rc) return rc;
            result.insert(result.end(), host.begin(), host.begin() + k);
            if (ctx->timing) ctx->last_ms[RK_MS_TOPN_HOST] += ms_since(t_host);
        }
    }
    rk_hit *out = (rk_hit *)malloc((result.empty() ? 1 : result.size()) * sizeof(rk_hit));
    if (!out) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %zu hits failed", result.size());
    if (!result.empty()) memcpy(out, result.data(), result.size() * sizeof(rk_hit));
    *hits_out = out;
    *n_hits = result.size();
    return RK_OK;
}
