// rk_greedy.hip -- greedy representatives of `alldist` on the device (rk_greedy_rows) and the same rule on the host over a hit list
// the caller already has (rk_greedy_hits).  The rule is greedy incremental clustering (CD-HIT; clust-greedy of RabbitTClust): walk the
// genomes in priority order -- (priority[a], a) ascending; without a priority the larger sketch first, then the caller index --; a
// genome is a REPRESENTATIVE unless a representative that precedes it is adjacent to it, otherwise a MEMBER of the nearest such
// representative (order of rk_edge_order.h; ties to the smallest caller index).  The graph is that of rk_cluster_rows.
//
//   stage     rk_edge_stage.h: the self join into a device buffer, its key pass (EdgeStage::key_pass<true>: per record w and
//             row << 32 | col; a BORDERLINE record goes, with its slot number, to the small host buffer and is dead for now; a record
//             outside 0 < common <= u -- multisets -- is counted: the call refuses such a collection), the two retries;
//   host      the stage decides the borderline records BEFORE any round (a kept edge can flip representatives arbitrarily far
//             away); the slot numbers of the kept ones go back up and k_edge_revive gives them their keys;
//   k_orient  per live record hi << 32 | lo: hi the endpoint of smaller rank (rank[] is the priority order, computed on the host);
//   rounds    k_edges: hi a representative -> lo is covered, the record dead; hi a member -> dead; hi and lo undecided -> lo is
//             blocked for this round.  k_vertices: an undecided genome that is covered becomes a member, one that is neither covered
//             nor blocked a representative, the others are counted.  The host reads the counters of a small batch of rounds and stops
//             at the first zero (a surplus round changes nothing);
//   assign    three sweeps over the records that took part, hi a representative and lo a member: atomic minimum of w per member,
//             atomic minimum of row << 32 | col among the records that match it, the winner writes rep[lo] and link[lo];
//   host      rep[] and link[] come home; links compacted to member order, jorc / dist recomputed with the C library's log.
//
// Why the rounds compute the sequential rule, and termination: DESIGN.md 4.8.  In short, by induction over the rank: a genome is
// decided in a round only when every adjacent genome of smaller rank was decided before the round began (else it is blocked) or one
// of them is a representative already (covered: a member whatever the others become); in both cases the sequential walk decides
// the same.  The undecided genome of smallest rank is never blocked, so every round decides at least one: N rounds at most.
// Memory scope: state[], covered[], blocked[], rank[], hl[], best_*[] and the key arrays are written by one kernel and read by a
// later one on the same stream (plain accesses behind kernel boundaries); the marks are same-value stores (covered: 1, blocked: the
// round's number); a record's hl[e] is touched by its own thread only.  The only communication inside a kernel is the two
// agent-scope relaxed minima of the assignment.  No loop waits for another workgroup: any grid works.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "rk_internal.h"
#include "rk_dist_plan.h"
#include "rk_edge_order.h"
#include "rk_edge_stage.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;      // rep[] of a genome nobody wrote yet
constexpr uint32_t kBatchMax = 8;            // rounds between two reads of the host

enum : uint32_t { kUndecided = 0, kRep = 1, kMember = 2 };

__global__ void k_greedy_init(uint32_t *state, uint32_t *covered, uint32_t *blocked, uint32_t *rep, unsigned long long *best_w,
                              unsigned long long *best_rc, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        state[i] = kUndecided;
        covered[i] = 0;
        blocked[i] = 0;   // (rounds count from 1)
        rep[i] = kNone;
        best_w[i] = kDead;
        best_rc[i] = kDead;
    }
}

// hi: the endpoint that precedes the other
__device__ __forceinline__ unsigned long long oriented(unsigned long long rc, const uint32_t *rank)
{
    const uint32_t a = (uint32_t)(rc >> 32), b = (uint32_t)rc;
    return rank[a] < rank[b] ? rc : ((unsigned long long)b << 32) | a;
}

__global__ void __launch_bounds__(kStageThreads)
k_greedy_orient(const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *rank, unsigned long long *hl)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x)
        hl[e] = w[e] == kDead ? kDead : oriented(rc[e], rank);
}

// state[] is the round's start: written by k_greedy_vertices / k_greedy_init, a kernel boundary away
__global__ void __launch_bounds__(kStageThreads)
k_greedy_edges(unsigned long long *hl, unsigned long long n_rec, const uint32_t *state, uint32_t *covered, uint32_t *blocked, uint32_t round)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long p = hl[e];
        if (p == kDead) continue;
        const uint32_t hi = (uint32_t)(p >> 32), lo = (uint32_t)p;
        const uint32_t s = state[hi];
        if (s == kRep) {
            covered[lo] = 1;
            hl[e] = kDead;
        } else if (s == kMember) {
            hl[e] = kDead;
        } else if (state[lo] == kUndecided) {
            blocked[lo] = round;
        }
    }
}

// the genomes still undecided behind this round go to *undecided, one atomic per wave
__global__ void __launch_bounds__(kStageThreads)
k_greedy_vertices(uint32_t *state, const uint32_t *covered, const uint32_t *blocked, uint32_t *rep, uint32_t n, uint32_t round, unsigned long long *undecided)
{
    uint32_t left = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (state[i] != kUndecided) continue;
        if (covered[i]) state[i] = kMember;
        else if (blocked[i] != round) {
            state[i] = kRep;
            rep[i] = i;
        } else left++;
    }
    for (int d = warpSize / 2; d > 0; d >>= 1) left += __shfl_down(left, d);
    if ((threadIdx.x & (warpSize - 1)) == 0 && left) atomicAdd(undecided, (unsigned long long)left);
}

// STEP 0: the best w per member; 1: among the records that match it, the best row << 32 | col; 2: the winner writes
template <int STEP>
__global__ void __launch_bounds__(kStageThreads)
k_greedy_assign(const rk_hit *hits, const unsigned long long *w, const unsigned long long *rc, unsigned long long n_rec, const uint32_t *rank,
                const uint32_t *state, unsigned long long *best_w, unsigned long long *best_rc, uint32_t *rep, rk_hit *link)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_rec; e += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long we = w[e];
        if (we == kDead) continue;
        const unsigned long long p = rc[e], o = oriented(p, rank);
        const uint32_t hi = (uint32_t)(o >> 32), lo = (uint32_t)o;
        if (state[hi] != kRep || state[lo] != kMember) continue;   // (a representative that comes later is not considered)
        if (STEP == 0) {
            min_u64(best_w + lo, we);
        } else if (STEP == 1) {
            if (best_w[lo] == we) min_u64(best_rc + lo, p);
        } else if (best_w[lo] == we && best_rc[lo] == p) {
            rep[lo] = hi;
            link[lo] = hits[e];
        }
    }
}

// rank[a] = the place of genome a in the priority order: (priority[a], a) ascending, or (-size[a], a) without a priority
void rank_of(const uint32_t *priority, const uint32_t *size, uint32_t n, std::vector<uint32_t> *rank)
{
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    if (priority) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return priority[a] < priority[b]; });
    else std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return size[a] > size[b]; });
    rank->resize(n);
    for (uint32_t k = 0; k < n; k++) (*rank)[order[k]] = k;
}

}  // namespace

extern "C" {

int rk_greedy_rows(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *opts, const uint32_t *priority, uint32_t *rep_out, rk_hit **links_out,
                   uint64_t *n_links, rk_greedy_stats *stats)
{
    if (!ctx || !idx || !opts) return RK_ERR_ARG;
    rk_greedy_stats st;
    memset(&st, 0, sizeof st);
    if (stats) *stats = st;
    if (!links_out || !n_links) return rk_fail(ctx, RK_ERR_ARG, "links_out or n_links is null");
    *links_out = nullptr;
    *n_links = 0;
    const uint32_t N = idx->n_ref;
    if (!rep_out && N) return rk_fail(ctx, RK_ERR_ARG, "rep_out is null");
    const StageNeeds needs{"rk_greedy_rows", "the greedy rule does not compose from row shards", true};
    if (int rc = stage_options(ctx, needs, opts)) return rc;
    if (!N) return RK_OK;
    if (int rc = stage_index(ctx, needs, idx, opts)) return rc;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    EdgeStage stage(ctx, idx, opts, needs.who, kPassGreedyKeys);   // with slot numbers
    const TimedSpan span{ctx, RK_MS_GREEDY_ROUNDS};
    const uint64_t max_rounds = (uint64_t)N + 1;   // every round with undecided genomes decides the first of them in rank order

    // the priority order, once: 4 * N bytes up (and, without a priority, the sizes and the genome order of the index down)
    std::vector<uint32_t> rank_h;
    if (priority) rank_of(priority, nullptr, N, &rank_h);
    else {
        std::vector<uint32_t> internal(N), size(N);
        RK_HIP(ctx, hipMemcpyAsync(internal.data(), idx->d_sizes, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
        if (idx->relabeled && idx->d_orig) {
            std::vector<uint32_t> orig(N);
            RK_HIP(ctx, hipMemcpyAsync(orig.data(), idx->d_orig, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
            RK_HIP(ctx, hipStreamSynchronize(stream));
            for (uint32_t i = 0; i < N; i++) {
                if (orig[i] >= N) return rk_fail(ctx, RK_ERR_HIP, "rk_greedy_rows: the index's genome order names genome %u of %u (internal error)", orig[i], N);
                size[orig[i]] = internal[i];
            }
        } else {
            RK_HIP(ctx, hipStreamSynchronize(stream));
            size.swap(internal);
        }
        rank_of(nullptr, size.data(), N, &rank_h);
    }

    DevBuf<uint32_t> rank(ctx), state(ctx), covered(ctx), blocked(ctx), rep(ctx);
    DevBuf<unsigned long long> best_w(ctx), best_rc(ctx), left_dev(ctx), w(ctx), rc_(ctx), hl(ctx);   // left_dev: the counters of a batch of rounds
    DevBuf<rk_hit> link(ctx);
    RK_HIP(ctx, rank.alloc(N));
    RK_HIP(ctx, state.alloc(N));
    RK_HIP(ctx, covered.alloc(N));
    RK_HIP(ctx, blocked.alloc(N));
    RK_HIP(ctx, rep.alloc(N));
    RK_HIP(ctx, best_w.alloc(N));
    RK_HIP(ctx, best_rc.alloc(N));
    RK_HIP(ctx, left_dev.alloc(kBatchMax));
    RK_HIP(ctx, link.alloc(N));
    RK_HIP(ctx, hipMemcpyAsync(rank.p, rank_h.data(), (size_t)N * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipStreamSynchronize(stream));   // (rank_h is pageable memory)
    hipLaunchKernelGGL(k_greedy_init, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, state.p, covered.p, blocked.p, rep.p, best_w.p, best_rc.p, N);
    RK_HIP(ctx, hipGetLastError());
    span.clear();

    // the key pass: nothing is decided before the stage is through
    int rc = stage.run([&](int pass) { return stage.key_pass<true>(pass, w, rc_, &hl); });
    if (rc) return rc;
    stage.stats(&st);
    // the borderline records, decided before any round
    if ((rc = stage.revive(w.p, &st.borderline_kept))) return rc;
    const rk_hit *hits = stage.hits.p;
    const unsigned long long n_rec = stage.n_hits;
    const unsigned grid = grid_for(ctx, n_rec);
    std::vector<uint32_t> rep_h(N);
    std::vector<rk_hit> link_h;
    if (stage.n_hits - stage.n_border + st.borderline_kept == 0) {   // no record takes part: no round, every genome its own representative
        std::iota(rep_h.begin(), rep_h.end(), 0u);
    } else {
        hipLaunchKernelGGL(k_greedy_orient, dim3(grid), dim3(kStageThreads), 0, stream, w.p, rc_.p, n_rec, rank.p, hl.p);
        RK_HIP(ctx, hipGetLastError());
        // decision rounds; the host reads the counters of a batch (one round at first: species cliques settle in two or three)
        RK_HIP(ctx, span.begin());
        uint64_t rounds = 0;
        bool settled = false;
        while (!settled) {
            const uint64_t batch = std::min<uint64_t>(rounds < 4 ? 1 : rounds < 16 ? 4 : kBatchMax, max_rounds - rounds);
            if (!batch) return rk_fail(ctx, RK_ERR_HIP, "rk_greedy_rows: %llu rounds did not decide %u genomes (internal error)", (unsigned long long)max_rounds, N);
            RK_HIP(ctx, hipMemsetAsync(left_dev.p, 0, batch * 8, stream));
            for (uint64_t b = 0; b < batch; b++) {
                const uint32_t round = (uint32_t)(rounds + b + 1);
                hipLaunchKernelGGL(k_greedy_edges, dim3(grid), dim3(kStageThreads), 0, stream, hl.p, n_rec, state.p, covered.p, blocked.p, round);
                hipLaunchKernelGGL(k_greedy_vertices, dim3(grid_for(ctx, N)), dim3(kStageThreads), 0, stream, state.p, covered.p, blocked.p, rep.p, N, round,
                                   left_dev.p + b);
            }
            RK_HIP(ctx, hipGetLastError());
            unsigned long long left[kBatchMax];
            if (int r = rk_read_back(ctx, left, left_dev.p, batch * 8, stream)) return r;
            uint64_t ran = batch;
            for (uint64_t b = 0; b < batch && !settled; b++)
                if (!left[b]) {
                    ran = b + 1;
                    settled = true;
                }
            rounds += ran;
        }
        st.rounds = (uint32_t)rounds;
        RK_HIP(ctx, span.end());
        // every member to its nearest preceding representative
        hipLaunchKernelGGL(k_greedy_assign<0>, dim3(grid), dim3(kStageThreads), 0, stream, hits, w.p, rc_.p, n_rec, rank.p, state.p, best_w.p, best_rc.p, rep.p, link.p);
        hipLaunchKernelGGL(k_greedy_assign<1>, dim3(grid), dim3(kStageThreads), 0, stream, hits, w.p, rc_.p, n_rec, rank.p, state.p, best_w.p, best_rc.p, rep.p, link.p);
        hipLaunchKernelGGL(k_greedy_assign<2>, dim3(grid), dim3(kStageThreads), 0, stream, hits, w.p, rc_.p, n_rec, rank.p, state.p, best_w.p, best_rc.p, rep.p, link.p);
        RK_HIP(ctx, hipGetLastError());
        link_h.resize(N);
        RK_HIP(ctx, hipMemcpyAsync(rep_h.data(), rep.p, (size_t)N * 4, hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipMemcpyAsync(link_h.data(), link.p, (size_t)N * sizeof(rk_hit), hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipStreamSynchronize(stream));
        span.read();
    }
    // links in member order (link_h[m] was written iff rep_h[m] != m; without a round there is none)
    uint64_t n_members = 0;
    for (uint32_t i = 0; i < N; i++) {
        if (rep_h[i] >= N) return rk_fail(ctx, RK_ERR_HIP, "rk_greedy_rows: genome %u was left without a representative (internal error)", i);
        if (rep_h[i] == i) continue;
        const rk_hit &h = link_h[i];
        if (!((h.row == i && h.col == rep_h[i]) || (h.col == i && h.row == rep_h[i])) || rep_h[rep_h[i]] != rep_h[i])
            return rk_fail(ctx, RK_ERR_HIP, "rk_greedy_rows: the link of genome %u does not join it to a representative (internal error)", i);
        link_h[n_members++] = h;   // (n_members <= i: nothing unread is overwritten)
    }
    // the reference's values bit for bit (a record that took part lies below the exact threshold: none is dropped)
    if (rk_host_exact_distances(link_h.data(), n_members, opts) != n_members)
        return rk_fail(ctx, RK_ERR_HIP, "rk_greedy_rows: a link lies beyond the exact threshold (internal error)");
    if (n_members) {
        rk_hit *out = host_records(n_members);
        if (!out) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu link records failed", (unsigned long long)n_members);
        memcpy(out, link_h.data(), n_members * sizeof(rk_hit));
        *links_out = out;
    }
    *n_links = n_members;
    memcpy(rep_out, rep_h.data(), (size_t)N * 4);
    st.n_reps = N - (uint32_t)n_members;
    if (stats) *stats = st;
    return RK_OK;
}

int rk_greedy_hits(const rk_hit *hits, uint64_t n_hits, uint32_t n, const uint32_t *priority, int metric, uint32_t *rep_out, rk_hit **links_out,
                   uint64_t *n_links)
{
    if ((n_hits && !hits) || (n && !rep_out) || !links_out || !n_links) return RK_ERR_ARG;
    *links_out = nullptr;
    *n_links = 0;
    metric = metric != 0;
    // the records: genomes below n, no loop, one size per genome; the adjacency as record numbers per genome
    std::vector<int64_t> seen(priority ? 0 : n, -1);
    for (uint64_t e = 0; e < n_hits; e++) {
        const rk_hit &h = hits[e];
        if (h.row >= n || h.col >= n || h.row == h.col) return RK_ERR_ARG;
        if (!priority) {
            if (h.size0 < 0 || h.size1 < 0) return RK_ERR_ARG;
            if ((seen[h.row] >= 0 && seen[h.row] != h.size0) || (seen[h.col] >= 0 && seen[h.col] != h.size1)) return RK_ERR_ARG;
            seen[h.row] = h.size0;
            seen[h.col] = h.size1;
        }
    }
    std::vector<uint32_t> rank;
    if (priority) rank_of(priority, nullptr, n, &rank);
    else {
        std::vector<uint32_t> size(n);
        for (uint32_t i = 0; i < n; i++) size[i] = seen[i] < 0 ? 0u : (uint32_t)seen[i];   // (a genome without a record is isolated: its place does not matter)
        rank_of(nullptr, size.data(), n, &rank);
    }
    std::vector<uint64_t> start, adj;
    hit_adjacency(hits, n_hits, n, &start, &adj);
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[rank[i]] = i;
    // the sequential rule
    const uint64_t none = ~0ULL;
    std::vector<uint64_t> link(n, none);
    std::vector<unsigned char> is_rep(n, 0);
    const EdgeLess nearer{metric};
    uint64_t n_members = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t v = order[k];
        rk_hit best{};
        for (uint64_t at = start[v]; at < start[v + 1]; at++) {
            const rk_hit &h = hits[adj[at]];
            const uint32_t other = h.row == v ? h.col : h.row;
            if (rank[other] > rank[v] || !is_rep[other]) continue;
            rk_hit x = h;   // ratio first, then the representative's index
            x.row = 0;
            x.col = other;
            if (link[v] == none || nearer(x, best)) {
                best = x;
                link[v] = adj[at];
            }
        }
        if (link[v] == none) {
            is_rep[v] = 1;
            rep_out[v] = v;
        } else {
            rep_out[v] = best.col;
            n_members++;
        }
    }
    if (n_members) {
        rk_hit *out = host_records(n_members);
        if (!out) return RK_ERR_NOMEM;
        uint64_t k = 0;
        for (uint32_t i = 0; i < n; i++)
            if (link[i] != none) out[k++] = hits[link[i]];
        *links_out = out;
    }
    *n_links = n_members;
    return RK_OK;
}

}  // extern "C"
