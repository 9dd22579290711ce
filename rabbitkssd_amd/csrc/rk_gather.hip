// rk_gather.hip -- which references explain a query sketch, in what order, and how much each adds beyond those already chosen
// (rk_gather_rows): the greedy minimum set cover of every selected query over the references of an index, and the same rule on the host
// over exported lists (rk_gather_lists).  Sketches are SETS.  Per query with hash set S: matched = the hashes of S with a posting list,
// common(r) = |S n R_r|, n_cand = the references with common >= min_new.  M_0 = the matched hashes; in round t rem_t(r) = |M_t n R_r|,
// the pick is the largest rem_t (ties: the smaller CALLER's index), the rounds end when it is below min_new or t = max_picks, else
// M_{t+1} = M_t \ R_pick.  include/rabbitkssd.h, decomposing queries into references.
//
// Per batch of query rows (as many counter rows as RK_GATHER_BATCH_BYTES holds), all on ctx->stream:
//   counts      rk_distq_counts (stage A of rk_dist_topn): int32 cnt[slot][N], columns in the caller's order.  These rows are the MUTABLE rem;
//   candidates  k_gather_candidates<false> counts the cells >= min_new of a row (n_cand), k_query_scan turns the counts into the rows'
//               regions, k_gather_candidates<true> compacts (common << 32 | ref) into them -- exact room, no retry; one reservation per wave;
//   match       k_gather_match: per query hash the index of its posting list (the look-up of rk_query_dev.h) or none; the hits are appended
//               as items slot << 32 | list (one reservation per wave) and counted per row (matched);
//   rounds      two kernels per round over the whole batch:
//               k_gather_pick   one workgroup per live row: the maximum of (rem, -ref) over the row's candidates, rem read from the
//                               counter row; candidates below min_new are dropped in place (the list only shrinks); the pick is appended
//                               to the row's region of min(max_picks, n_cand) records, the winner's INTERNAL id kept (the inverse of
//                               d_orig, built once per call); a row without a candidate, at max_picks or with nothing left retires;
//               k_gather_cover  one lane per live item: a binary search of the row's winner in postings[upos[u] .. upos[u + 1]) (a list
//                               ascends in internal id: rk_index_build sorts (hash, genome), an import keeps the .dict order, which
//                               rk_group.hip's repeat test relies on as well).  On a hit the list dies and every posting of it takes an
//                               atomic -1 on rem[row][orig[p]] -- by the lane itself up to lane_max postings, by its wave up to wave_max,
//                               by the workgroup (an LDS queue) beyond.  A list dies at most once: the decrements of a batch total at
//                               most the postings under its matched lists;
//               the items are compacted (k_gather_compact) when fewer than half are alive;
//   picks       k_query_scan over the rows' pick counts + k_gather_take: the batch's picks in (query, rank) order;
//   result      off[Q + 1] by k_query_scan over all rows; ONE copy to the host: 8 (Q + 1) + 12 Q + 32 picks bytes.
//
// Termination: a round either appends a pick with fresh >= min_new >= 1 or retires the row, and a pick takes fresh hashes out of M, so a
// row makes at most min(max_picks, matched, N) picks and retires in the round after its last one at the latest: the host launches at
// most min(max_picks, largest query of the batch, N) + 1 rounds.  It reads the counter of live rows every sync_every rounds
// (RK_GATHER_SYNC_EVERY, default 4: DESIGN.md 4.15) and launches nothing once it is 0.
//
// Memory scope: every array is written by one kernel and read by a later one on the same stream.  INSIDE a launch the only communication
// is relaxed agent-scope atomic adds -- the -1 on the counter rows (nobody reads rem in k_gather_cover), the reservations and the
// statistics -- and LDS between barriers.  No loop waits for another workgroup: any grid works.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_internal.h"
#include "rk_query_dev.h"
#include "rk_query_host.h"

namespace {

constexpr uint32_t kNoWinner = 0xFFFFFFFFu;
constexpr unsigned long long kDeadItem = ~0ULL;
constexpr int kGatherThreads = 256;
constexpr uint32_t kLaneMax = 16;    // k_gather_cover: the longest list the lane that found the winner walks itself (RK_GATHER_LANE_MAX)
constexpr uint32_t kWaveMax = 256;   // the longest list its wave walks (64 postings per trip); beyond: the workgroup
constexpr uint32_t kSyncEvery = 4;   // rounds between two reads of the live-row counter
static_assert(sizeof(rk_gather_opts) == 20 && sizeof(rk_gather_pick) == 32 && sizeof(rk_gather_stats) == 112, "the layouts of include/rabbitkssd.h");

struct Counters {   // one device block, read back in one copy
    unsigned long long live_rows, n_items, dead_items, n_compacted, picks, decrements, lane_lists, wave_lists, block_lists;
    unsigned long long cand_total, region_total, take_total;
};

struct RowArgs {   // a batch of nb rows: slot s of the batch is query row row_of[s], its counter row cnt + s * n_ref
    int32_t *cnt;
    const uint32_t *row_of;
    uint32_t n_ref, min_new, max_picks;
    uint32_t *n_cand_q, *matched_q, *covered_q, *npicks_q;   // per QUERY row (the call's outputs)
    const unsigned long long *cand_off, *pick_off;           // per slot: nb + 1 each
    unsigned long long *cand;                                // common << 32 | ref (caller's index)
    uint32_t *cand_len, *left, *winner, *done;               // per slot
    rk_gather_pick *picks;
    const uint32_t *inv, *sizes;                             // per caller's reference index
    const uint64_t *q_off;
    Counters *c;
};

// One workgroup per row.  WRITE false: n_cand = the cells of the counter row at or above min_new.  WRITE true: those cells compacted
// into the row's region (its exact size: the scan of the counts), in any order -- one LDS reservation per wave.
template <bool WRITE> __global__ void __launch_bounds__(kGatherThreads) k_gather_candidates(RowArgs a)
{
    __shared__ uint32_t s_fill;
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63;
    const int32_t *cnt = a.cnt + (size_t)s * a.n_ref;
    if (tid == 0) s_fill = 0;
    __syncthreads();
    const unsigned long long beg = WRITE ? a.cand_off[s] : 0ULL, room = WRITE ? a.cand_off[s + 1] - beg : 0ULL;
    uint32_t mine = 0;
    for (uint32_t c0 = 0; c0 < a.n_ref; c0 += kGatherThreads) {   // (uniform)
        const uint32_t c = c0 + tid;
        const uint32_t v = c < a.n_ref ? (uint32_t)cnt[c] : 0u;
        const bool keep = v >= a.min_new;   // (min_new >= 1)
        if (WRITE) {
            const unsigned long long m = __ballot(keep);
            if (m) {   // (uniform in the wave)
                const int lead = __ffsll((long long)m) - 1;
                uint32_t base = 0;
                if (lane == lead) base = atomicAdd(&s_fill, (uint32_t)__popcll(m));
                const unsigned long long at = (uint32_t)__shfl((int)base, lead) + (uint32_t)__popcll(m & lanes_below(lane));
                if (keep && at < room) a.cand[beg + at] = ((unsigned long long)v << 32) | c;
            }
        } else {
            mine += keep;
        }
    }
    if (!WRITE) {
        if (mine) atomicAdd(&s_fill, mine);
        __syncthreads();
        if (tid == 0) a.n_cand_q[a.row_of[s]] = s_fill;
    }
}

struct MatchArgs {
    const void *q_hashes;
    const uint64_t *q_off;
    const uint32_t *row_of;
    IndexLookup ix;
    unsigned long long *items, cap;
    uint32_t *matched_q;
    Counters *c;
};

// One workgroup per row, one query hash per lane and trip: a hash that has a posting list appends the item slot << 32 | list.
template <class Hash> __global__ void __launch_bounds__(kGatherThreads) k_gather_match(MatchArgs a)
{
    __shared__ uint32_t s_n;
    const uint32_t s = blockIdx.x, tid = threadIdx.x, row = a.row_of[s];
    const Hash *q = (const Hash *)a.q_hashes;
    const uint64_t qb = a.q_off[row], qe = a.q_off[row + 1];
    if (tid == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint64_t j0 = qb; j0 < qe; j0 += kGatherThreads) {   // (uniform)
        const uint64_t j = j0 + tid;
        const bool in[1] = {j < qe};
        const unsigned long long h[1] = {in[0] ? (unsigned long long)q[j] : 0ULL};
        uint32_t u[1];
        index_lookup<Hash, 1>(a.ix, h, in, u);
        const bool found = u[0] != kNoList;
        wave_append(found, ((unsigned long long)s << 32) | u[0], &a.c->n_items, a.items, a.cap);
        mine += found;
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0) a.matched_q[row] = s_n;
}

// the state of the rows before round 0; every row starts alive (one without a candidate retires in round 0)
__global__ void k_gather_init(RowArgs a, uint32_t nb)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nb) return;
    const uint32_t row = a.row_of[s];
    a.cand_len[s] = a.n_cand_q[row];
    a.left[s] = a.matched_q[row];
    a.winner[s] = kNoWinner;
    a.done[s] = 0;
    if (s == 0) a.c->live_rows = nb;
}

// One workgroup per row of the batch; a retired row returns at once.
__global__ void __launch_bounds__(kGatherThreads) k_gather_pick(RowArgs a)
{
    __shared__ uint32_t s_cnt[kGatherThreads / 64], s_common[kGatherThreads / 64];
    __shared__ unsigned long long s_key[kGatherThreads / 64];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    if (a.done[s]) return;   // (uniform)
    const int32_t *rem = a.cnt + (size_t)s * a.n_ref;
    unsigned long long *cand = a.cand + a.cand_off[s];
    const uint32_t n = a.cand_len[s];
    unsigned long long best = 0;   // rem << 32 | ~ref: a kept candidate has rem >= 1
    uint32_t best_common = 0, base = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += kGatherThreads) {   // (uniform)
        const uint32_t i = c0 + tid;
        unsigned long long e = 0;
        bool keep = false;
        if (i < n) {
            e = cand[i];
            const uint32_t ref = (uint32_t)e, r = (uint32_t)rem[ref];   // (ref < n_ref: k_gather_candidates wrote a column)
            keep = r >= a.min_new && r <= (uint32_t)INT_MAX;
            const unsigned long long key = ((unsigned long long)r << 32) | (uint32_t)~ref;
            if (keep && key > best) {
                best = key;
                best_common = (uint32_t)(e >> 32);
            }
        }
        // the survivors move to the front: every entry of this chunk has been read, a target lies at or before its source
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kGatherThreads / 64; k++) {
            if (k < w) before += s_cnt[k];
            all += s_cnt[k];
        }
        const uint32_t at = base + before + (uint32_t)__popcll(m & lanes_below(lane));
        if (keep && at != i) cand[at] = e;
        base += all;
        __syncthreads();   // (s_cnt is rewritten, and the next chunk's reads follow this chunk's writes)
    }
    unsigned long long top = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = shfl_xor_u64(top, o);
        if (x > top) top = x;
    }
    if (lane == 0) s_key[w] = top;
    if (best == top && top) s_common[w] = best_common;   // (keys are distinct: one lane)
    __syncthreads();
    if (tid != 0) return;
    int bw = 0;
    for (int k = 1; k < kGatherThreads / 64; k++)
        if (s_key[k] > s_key[bw]) bw = k;
    top = s_key[bw];
    a.cand_len[s] = base;
    const uint32_t row = a.row_of[s], t = a.npicks_q[row];
    const unsigned long long room = a.pick_off[s + 1] - a.pick_off[s];
    bool retire = !top || t >= room;   // (t < room whenever a candidate is left: room = min(max_picks, n_cand))
    if (!retire) {
        const uint32_t fresh = (uint32_t)(top >> 32), ref = ~(uint32_t)top, left = a.left[s] - fresh;
        rk_gather_pick p;
        p.query = row;
        p.ref = ref;
        p.rank = t;
        p.common = s_common[bw];
        p.fresh = fresh;
        p.left = left;
        p.size_ref = a.sizes[ref];
        p.size_query = (uint32_t)(a.q_off[row + 1] - a.q_off[row]);
        a.picks[a.pick_off[s] + t] = p;
        a.left[s] = left;
        a.covered_q[row] += fresh;
        a.npicks_q[row] = t + 1;
        add_u64(&a.c->picks, 1ULL);
        a.winner[s] = a.inv[ref];
        retire = (a.max_picks && t + 1 >= a.max_picks) || left == 0;   // nothing more to pick: no cover needed either
    }
    if (retire) {
        a.winner[s] = kNoWinner;
        a.done[s] = 1;
        add_u64(&a.c->live_rows, ~0ULL);   // -1
    }
}

struct CoverArgs {
    int32_t *cnt;
    const uint32_t *postings, *upos, *orig;   // orig null: the identity
    const uint32_t *winner, *done;
    unsigned long long *items, n_items;
    uint32_t n_ref, lane_max, wave_max;
    Counters *c;
};

__device__ __forceinline__ void take_one(int32_t *rem, const uint32_t *orig, uint32_t p)
{
    __hip_atomic_fetch_add(rem + (orig ? orig[p] : p), -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per item.  The item of a retired row dies; the item of a live row whose list holds the row's winner dies and its postings
// are taken off the row's rem -- by this lane, by its wave or by the workgroup, by the length of the list.
__global__ void __launch_bounds__(kGatherThreads) k_gather_cover(CoverArgs a)
{
    __shared__ uint32_t s_qn, s_qbeg[kGatherThreads], s_qlen[kGatherThreads], s_qslot[kGatherThreads];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63;
    if (tid == 0) s_qn = 0;
    __syncthreads();
    const unsigned long long i = (unsigned long long)blockIdx.x * kGatherThreads + tid;
    const unsigned long long item = i < a.n_items ? a.items[i] : kDeadItem;
    const bool alive = item != kDeadItem;
    const uint32_t s = alive ? (uint32_t)(item >> 32) : 0u, u = (uint32_t)item;
    bool die = false, hit = false;
    uint32_t beg = 0, len = 0;
    if (alive) {
        if (a.done[s]) {
            die = true;
        } else {
            const uint32_t win = a.winner[s];   // (a live row behind k_gather_pick has a winner)
            beg = a.upos[u];
            len = a.upos[u + 1] - beg;
            uint32_t lo = 0, hi = len;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.postings[beg + mid] < win) lo = mid + 1; else hi = mid;
            }
            hit = win != kNoWinner && lo < len && a.postings[beg + lo] == win;
            die = hit;
        }
        if (die) a.items[i] = kDeadItem;
    }
    int32_t *rem = a.cnt + (size_t)s * a.n_ref;
    const bool by_lane = hit && len <= a.lane_max, by_wave = hit && !by_lane && len <= a.wave_max, by_block = hit && !by_lane && !by_wave;
    if (by_lane)
        for (uint32_t j = 0; j < len; j++) take_one(rem, a.orig, a.postings[beg + j]);
    unsigned long long pending = __ballot(by_wave);
    while (pending) {   // (uniform in the wave)
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        const uint32_t b = (uint32_t)__shfl((int)beg, src), l = (uint32_t)__shfl((int)len, src), sl = (uint32_t)__shfl((int)s, src);
        int32_t *r = a.cnt + (size_t)sl * a.n_ref;
        for (uint32_t j = lane; j < l; j += 64) take_one(r, a.orig, a.postings[b + j]);
    }
    if (by_block) {
        const uint32_t at = atomicAdd(&s_qn, 1u);   // (at most one per thread: at < kGatherThreads)
        s_qbeg[at] = beg;
        s_qlen[at] = len;
        s_qslot[at] = s;
    }
    __syncthreads();
    const uint32_t qn = s_qn;
    for (uint32_t k = 0; k < qn; k++) {   // (uniform)
        int32_t *r = a.cnt + (size_t)s_qslot[k] * a.n_ref;
        const uint32_t b = s_qbeg[k], l = s_qlen[k];
        for (uint32_t j = tid; j < l; j += kGatherThreads) take_one(r, a.orig, a.postings[b + j]);
    }
    // the statistics: one atomic per wave and counter that moved
    const unsigned long long m_die = __ballot(die), m_lane = __ballot(by_lane), m_wave = __ballot(by_wave), m_block = __ballot(by_block);
    if (!m_die) return;   // (uniform in the wave)
    unsigned long long walked = hit ? len : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) walked += shfl_xor_u64(walked, o);
    if (lane == 0) {
        add_u64(&a.c->dead_items, (unsigned long long)__popcll(m_die));
        if (walked) add_u64(&a.c->decrements, walked);
        if (m_lane) add_u64(&a.c->lane_lists, (unsigned long long)__popcll(m_lane));
        if (m_wave) add_u64(&a.c->wave_lists, (unsigned long long)__popcll(m_wave));
        if (m_block) add_u64(&a.c->block_lists, (unsigned long long)__popcll(m_block));
    }
}

// the live items, in any order, behind *counter
__global__ void __launch_bounds__(kGatherThreads) k_gather_compact(const unsigned long long *items, unsigned long long n, unsigned long long *out,
                                                                   unsigned long long cap, unsigned long long *counter)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kGatherThreads + threadIdx.x;
    const unsigned long long item = i < n ? items[i] : kDeadItem;
    wave_append(item != kDeadItem, item, counter, out, cap);
}

// the picks of the batch's rows, back to back in (row, rank) order: take_off = k_query_scan over the rows' pick counts
__global__ void __launch_bounds__(kGatherThreads) k_gather_take(RowArgs a, const unsigned long long *take_off, rk_gather_pick *out)
{
    const uint32_t s = blockIdx.x;
    const unsigned long long n = take_off[s + 1] - take_off[s];
    const rk_gather_pick *src = a.picks + a.pick_off[s];
    for (unsigned long long k = threadIdx.x; k < n; k += kGatherThreads) out[take_off[s] + k] = src[k];
}

// ---- host: the rule, exactly ------------------------------------------------------------------------------------------------
struct HostResult {
    std::vector<rk_gather_pick> picks;
    std::vector<uint64_t> off;                          // Q + 1
    std::vector<uint32_t> matched, n_cand, covered;     // Q (unselected rows: 0)
};

// lists: list u is post[pos[u] .. pos[u + 1]), strictly ascending reference ids below n_ref
void gather_core(const uint32_t *post, const uint64_t *pos, const uint64_t *q_off, const uint64_t *q_lists, uint32_t Q, uint32_t n_ref,
                 const uint32_t *ref_sizes, const uint32_t *query_sizes, const rk_gather_opts *o, const RowSel &sel, HostResult *out)
{
    std::vector<uint32_t> rem(n_ref, 0), common(n_ref, 0), touched, cands;
    std::vector<uint64_t> start(n_ref, 0);
    std::vector<uint32_t> by_ref;     // per touched reference the local numbers of the lists that hold it
    std::vector<uint8_t> alive;
    std::vector<uint32_t> n_picks(Q, 0);
    out->matched.assign(Q, 0);
    out->n_cand.assign(Q, 0);
    out->covered.assign(Q, 0);
    for (const uint32_t q : sel.rows) {
        const uint64_t *lists = q_lists + q_off[q];
        const uint64_t nl = q_off[q + 1] - q_off[q];
        touched.clear();
        uint32_t matched = 0;
        uint64_t total = 0;
        for (uint64_t k = 0; k < nl; k++) {
            const uint64_t u = lists[k];
            matched += pos[u + 1] > pos[u];   // (an empty list matches nothing)
            for (uint64_t i = pos[u]; i < pos[u + 1]; i++)
                if (!rem[post[i]]++) touched.push_back(post[i]);
            total += pos[u + 1] - pos[u];
        }
        uint64_t at = 0;
        for (const uint32_t r : touched) {
            common[r] = rem[r];
            start[r] = at;
            at += rem[r];
        }
        by_ref.resize(total);
        for (uint64_t k = 0; k < nl; k++)
            for (uint64_t i = pos[lists[k]]; i < pos[lists[k] + 1]; i++) by_ref[start[post[i]]++] = (uint32_t)k;
        for (const uint32_t r : touched) start[r] -= common[r];
        alive.assign(nl, 1);
        cands.clear();
        for (const uint32_t r : touched)
            if (common[r] >= o->min_new) cands.push_back(r);
        const uint32_t n_cand = (uint32_t)cands.size();
        uint32_t left = matched, covered = 0, t = 0;
        while (!o->max_picks || t < o->max_picks) {
            uint32_t best = 0, best_ref = 0;
            size_t keep = 0;
            for (const uint32_t r : cands) {
                if (rem[r] < o->min_new) continue;   // rem only falls: out for good
                cands[keep++] = r;
                if (rem[r] > best || (rem[r] == best && r < best_ref)) {
                    best = rem[r];
                    best_ref = r;
                }
            }
            cands.resize(keep);
            if (!best) break;
            left -= best;
            covered += best;
            out->picks.push_back(rk_gather_pick{q, best_ref, t, common[best_ref], best, left, ref_sizes[best_ref], query_sizes[q]});
            t++;
            for (uint64_t j = start[best_ref]; j < start[best_ref] + common[best_ref]; j++) {
                const uint32_t k = by_ref[j];
                if (!alive[k]) continue;
                alive[k] = 0;
                for (uint64_t i = pos[lists[k]]; i < pos[lists[k] + 1]; i++) rem[post[i]]--;
            }
        }
        for (const uint32_t r : touched) rem[r] = 0;
        n_picks[q] = t;
        out->matched[q] = matched;
        out->n_cand[q] = n_cand;
        out->covered[q] = covered;
    }
    out->off.assign((size_t)Q + 1, 0);
    for (uint32_t q = 0; q < Q; q++) out->off[q + 1] = out->off[q] + n_picks[q];
}

using Result = RowsResult<rk_gather_pick, 3>;   // per row: matched, n_cand, covered

Result view(const HostResult &r)
{
    return Result{r.off.data(), {r.matched.data(), r.n_cand.data(), r.covered.data()}, r.picks.data(), r.picks.size()};
}

void fill_constants(rk_gather_stats *st, uint32_t lane_max, uint32_t wave_max, uint32_t sync_every)
{
    st->lane_max = lane_max;
    st->wave_max = wave_max;
    st->sync_every = sync_every;
    st->threads = kGatherThreads;
}

unsigned long long env_number(const char *name, unsigned long long otherwise)
{
    const char *sw = getenv(name);
    const unsigned long long v = sw ? strtoull(sw, nullptr, 10) : 0;
    return v ? v : otherwise;
}

// RK_GATHER_DEVICE=0: export + the lists of the selected queries' hashes (a binary search each) + the rule on the host
template <class Hash> int gather_on_host(rk_ctx *ctx, const rk_index *idx, const rk_sketches *qs, const rk_gather_opts *o, const RowSel &sel, HostResult *out)
{
    const uint32_t N = idx->n_ref, Q = qs->n;
    std::vector<uint32_t> postings(idx->H), counts(idx->U), ref_sizes(N), query_sizes(Q);
    std::vector<Hash> hashes(idx->U), qh(qs->total);
    std::vector<uint64_t> qoff((size_t)Q + 1);
    if constexpr (sizeof(Hash) == 8) {
        RK_TRY(rk_index_export64(idx, postings.data(), hashes.data(), counts.data()));
        RK_TRY(rk_sketches_download64(qs, qh.data(), qoff.data()));
    } else {
        RK_TRY(rk_index_export_lists(idx, postings.data(), hashes.data(), counts.data()));
        RK_TRY(rk_sketches_download(qs, qh.data(), qoff.data()));
    }
    {   // the sizes the index carries (an import: the caller's), in the caller's order
        std::vector<uint32_t> sizes(N), orig(N);
        RK_TRY(rk_index_order(idx, orig.data()));
        RK_HIP(ctx, hipMemcpyAsync(sizes.data(), idx->d_sizes, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
        RK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = 0; i < N; i++) ref_sizes[orig[i] < N ? orig[i] : i] = sizes[i];
    }
    std::vector<uint64_t> l_off((size_t)Q + 1, 0), l;
    size_t next = 0;
    for (uint32_t q = 0; q < Q; q++) {
        query_sizes[q] = (uint32_t)(qoff[q + 1] - qoff[q]);
        if (next < sel.rows.size() && sel.rows[next] == q) {
            next++;
            for (uint64_t j = qoff[q]; j < qoff[q + 1]; j++) {
                const auto it = std::lower_bound(hashes.begin(), hashes.end(), qh[j]);
                if (it != hashes.end() && *it == qh[j]) l.push_back((uint64_t)(it - hashes.begin()));
            }
        }
        l_off[q + 1] = l.size();
    }
    std::vector<uint64_t> pos;
    std::vector<uint32_t> fixed;
    const uint32_t *post = nullptr;
    if (prepare_lists(postings.data(), counts.data(), idx->U, N, &pos, &fixed, &post))
        return rk_fail(ctx, RK_ERR_HIP, "rk_gather_rows: an exported posting names a genome beyond their number (internal error)");
    gather_core(post, pos.data(), l_off.data(), l.data(), Q, N, ref_sizes.data(), query_sizes.data(), o, sel, out);
    return RK_OK;
}

struct DeviceResult {
    std::vector<unsigned char> block;   // Result::from_block
    uint64_t n_picks = 0;
};

int gather_on_device(rk_ctx *ctx, const rk_index *idx, const rk_sketches *qs, const rk_gather_opts *o, const RowSel &sel, rk_gather_stats *st, DeviceResult *res)
{
    const uint32_t N = idx->n_ref, Q = qs->n;
    const uint64_t n_sel = sel.rows.size();
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const TimedSpan span{ctx, RK_MS_GATHER};
    const uint32_t lane_max = st->lane_max, wave_max = st->wave_max, sync_every = st->sync_every;
    RK_TRY(rk_index_ensure_dir(ctx, const_cast<rk_index *>(idx), stream));
    rk_dist_opts dopts;   // the row shard for rk_distq_counts; nothing of a distance is evaluated
    memset(&dopts, 0, sizeof dopts);
    dopts.kmer_size = 1;
    dopts.max_dist = 1.0;
    dopts.row_block = (int32_t)std::min<uint32_t>(o->row_block, (uint32_t)INT_MAX);
    dopts.row_first = o->row_first;
    dopts.row_step = o->row_step;

    DevBuf<uint32_t> per_q(ctx), inv(ctx), sizes(ctx), row_of(ctx), per_slot(ctx);
    DevBuf<Counters> cnt_dev(ctx);
    DevBuf<unsigned long long> offs(ctx), items(ctx), cand(ctx);
    DevBuf<int32_t> counts(ctx);
    DevBuf<rk_gather_pick> picks(ctx);
    RK_HIP(ctx, per_q.alloc((size_t)4 * Q));   // n_cand, matched, covered, npicks
    RK_HIP(ctx, inv.alloc(N));
    RK_HIP(ctx, sizes.alloc(N));
    RK_HIP(ctx, cnt_dev.alloc(1));
    RK_HIP(ctx, hipMemsetAsync(per_q.p, 0, (size_t)16 * Q, stream));
    RK_HIP(ctx, span.begin());
    hipLaunchKernelGGL(k_query_prepare, dim3(blocks_for(N)), dim3(kThreads), 0, stream, idx->relabeled ? idx->d_orig : nullptr, idx->d_sizes, N, inv.p, sizes.p);
    RK_HIP(ctx, hipGetLastError());
    st->launches++;

    // device bytes of one row of a batch: its counter row, its candidates, its items (twice: the compaction's target) and its state
    const uint64_t row_bytes = (uint64_t)N * 12 + qs->max_size * 16 + 64;
    const uint64_t rows_per_batch = std::max<uint64_t>(1, std::min<uint64_t>(n_sel, env_number("RK_GATHER_BATCH_BYTES", 1ULL << 30) / row_bytes));
    st->rows_per_batch = rows_per_batch;
    RK_HIP(ctx, counts.alloc(rows_per_batch * N));
    RK_HIP(ctx, row_of.alloc(rows_per_batch));
    RK_HIP(ctx, per_slot.alloc(4 * rows_per_batch));        // cand_len, left, winner, done
    RK_HIP(ctx, offs.alloc(3 * (rows_per_batch + 1)));      // cand_off, pick_off, take_off

    struct Taken {   // the picks of one batch, in order, until the result is put together
        rk_ctx *ctx;
        std::vector<std::pair<rk_gather_pick *, uint64_t>> parts;
        ~Taken() { for (auto &p : parts) rk_pool_free(ctx, p.first); }
    } taken{ctx, {}};
    uint64_t total_picks = 0;

    for (uint64_t s0 = 0; s0 < n_sel; s0 += rows_per_batch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(rows_per_batch, n_sel - s0);
        st->batches++;
        uint64_t hashes = 0, biggest = 0;
        for (uint32_t s = 0; s < nb; s++) {
            const uint64_t size = qs->h_off[sel.rows[s0 + s] + 1] - qs->h_off[sel.rows[s0 + s]];
            hashes += size;
            biggest = std::max(biggest, size);
        }
        RK_TRY(rk_distq_counts(ctx, idx, qs, &dopts, (uint32_t)s0, nb, counts.p, stream));
        // (pageable memory of the caller's vector: the read-back of the counters below synchronises the stream)
        RK_HIP(ctx, hipMemcpyAsync(row_of.p, sel.rows.data() + s0, (size_t)nb * 4, hipMemcpyHostToDevice, stream));
        RK_HIP(ctx, hipMemsetAsync(cnt_dev.p, 0, sizeof(Counters), stream));
        RK_HIP(ctx, items.alloc(2 * hashes));
        RowArgs a;
        memset(&a, 0, sizeof a);
        a.cnt = counts.p;
        a.row_of = row_of.p;
        a.n_ref = N;
        a.min_new = o->min_new;
        a.max_picks = o->max_picks;
        a.n_cand_q = per_q.p;
        a.matched_q = per_q.p + Q;
        a.covered_q = per_q.p + 2 * (size_t)Q;
        a.npicks_q = per_q.p + 3 * (size_t)Q;
        a.cand_off = offs.p;
        a.pick_off = offs.p + (rows_per_batch + 1);
        unsigned long long *take_off = offs.p + 2 * (rows_per_batch + 1);
        a.cand_len = per_slot.p;
        a.left = per_slot.p + rows_per_batch;
        a.winner = per_slot.p + 2 * rows_per_batch;
        a.done = per_slot.p + 3 * rows_per_batch;
        a.inv = inv.p;
        a.sizes = sizes.p;
        a.q_off = qs->d_off;
        a.c = cnt_dev.p;
        hipLaunchKernelGGL(k_gather_candidates<false>, dim3(nb), dim3(kGatherThreads), 0, stream, a);
        if (hashes && idx->U) {
            MatchArgs m;
            m.q_hashes = qs->wide ? (const void *)qs->d_hashes64 : (const void *)qs->d_hashes;
            m.q_off = qs->d_off;
            m.row_of = row_of.p;
            m.ix = index_lookup_of(idx);
            m.items = items.p;
            m.cap = hashes;
            m.matched_q = a.matched_q;
            m.c = cnt_dev.p;
            if (idx->wide) hipLaunchKernelGGL(k_gather_match<uint64_t>, dim3(nb), dim3(kGatherThreads), 0, stream, m);
            else hipLaunchKernelGGL(k_gather_match<uint32_t>, dim3(nb), dim3(kGatherThreads), 0, stream, m);
            st->launches++;
        }
        hipLaunchKernelGGL(k_query_scan<kGatherThreads>, dim3(1), dim3(kGatherThreads), 0, stream, a.n_cand_q, row_of.p, nb, 0u, offs.p, &cnt_dev.p->cand_total);
        hipLaunchKernelGGL(k_query_scan<kGatherThreads>, dim3(1), dim3(kGatherThreads), 0, stream, a.n_cand_q, row_of.p, nb, o->max_picks, offs.p + (rows_per_batch + 1),
                           &cnt_dev.p->region_total);
        hipLaunchKernelGGL(k_gather_init, dim3(blocks_for(nb)), dim3(kThreads), 0, stream, a, nb);
        RK_HIP(ctx, hipGetLastError());
        st->launches += 4;
        Counters home;
        RK_TRY(rk_read_back(ctx, &home, cnt_dev.p, sizeof home, stream));   // the room of the candidates and of the picks
        st->read_backs++;
        if (home.n_items > hashes || home.cand_total > (unsigned long long)nb * N || home.region_total > home.cand_total)
            return rk_fail(ctx, RK_ERR_HIP, "rk_gather_rows: more matched hashes or candidates than there are hashes or cells (internal error)");
        RK_HIP(ctx, cand.alloc(home.cand_total));
        RK_HIP(ctx, picks.alloc(home.region_total));
        a.cand = cand.p;
        a.picks = picks.p;
        if (home.cand_total) {
            hipLaunchKernelGGL(k_gather_candidates<true>, dim3(nb), dim3(kGatherThreads), 0, stream, a);
            RK_HIP(ctx, hipGetLastError());
            st->launches++;
        }
        // the rounds
        const uint64_t bound = std::min<uint64_t>(std::min<uint64_t>(o->max_picks ? o->max_picks : UINT_MAX, biggest), N);
        unsigned long long live = nb, n_cur = home.n_items, dead_before = 0, compacted_to = ~0ULL;   // compacted_to: what the last compaction must have kept
        unsigned long long *cur = items.p, *other = items.p + hashes;
        CoverArgs c;
        c.cnt = counts.p;
        c.postings = idx->d_postings;
        c.upos = idx->d_upos;
        c.orig = idx->relabeled ? idx->d_orig : nullptr;
        c.winner = a.winner;
        c.done = a.done;
        c.n_ref = N;
        c.lane_max = lane_max;
        c.wave_max = wave_max;
        c.c = cnt_dev.p;
        for (uint64_t t = 0; live && t <= bound;) {
            hipLaunchKernelGGL(k_gather_pick, dim3(nb), dim3(kGatherThreads), 0, stream, a);
            st->launches++;
            if (n_cur) {
                c.items = cur;
                c.n_items = n_cur;
                hipLaunchKernelGGL(k_gather_cover, dim3(blocks_for(n_cur, kGatherThreads)), dim3(kGatherThreads), 0, stream, c);
                st->launches++;
            }
            RK_HIP(ctx, hipGetLastError());
            t++;
            st->launched_rounds++;
            if (t % sync_every && t <= bound) continue;
            RK_TRY(rk_read_back(ctx, &home, cnt_dev.p, sizeof home, stream));
            st->read_backs++;
            live = home.live_rows;
            if (live > nb || home.dead_items - dead_before > n_cur || (compacted_to != ~0ULL && home.n_compacted != compacted_to))
                return rk_fail(ctx, RK_ERR_HIP, "rk_gather_rows: the counters of live rows and lists left their range (internal error)");
            const unsigned long long alive = n_cur - (home.dead_items - dead_before);
            if (live && alive * 2 < n_cur) {   // fewer than half survive: the next rounds walk the survivors only
                RK_HIP(ctx, hipMemsetAsync(&cnt_dev.p->n_compacted, 0, 8, stream));
                hipLaunchKernelGGL(k_gather_compact, dim3(blocks_for(n_cur, kGatherThreads)), dim3(kGatherThreads), 0, stream, cur, n_cur, other, hashes,
                                   &cnt_dev.p->n_compacted);
                RK_HIP(ctx, hipGetLastError());
                st->launches++;
                st->compactions++;
                std::swap(cur, other);
                n_cur = compacted_to = alive;   // (exact: the read-back followed the last cover)
                dead_before = home.dead_items;
            }
        }
        if (live) return rk_fail(ctx, RK_ERR_HIP, "rk_gather_rows: rows are alive after the last possible round (internal error)");
        if (home.picks > home.region_total) return rk_fail(ctx, RK_ERR_HIP, "rk_gather_rows: more picks than their room (internal error)");
        st->decrements += home.decrements;
        st->lane_lists += home.lane_lists;
        st->wave_lists += home.wave_lists;
        st->block_lists += home.block_lists;
        if (home.picks) {
            rk_gather_pick *part = static_cast<rk_gather_pick *>(rk_pool_alloc(ctx, home.picks * sizeof(rk_gather_pick)));
            if (!part) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu picks on the device", home.picks);
            taken.parts.emplace_back(part, home.picks);
            hipLaunchKernelGGL(k_query_scan<kGatherThreads>, dim3(1), dim3(kGatherThreads), 0, stream, a.npicks_q, row_of.p, nb, 0u, take_off, &cnt_dev.p->take_total);
            hipLaunchKernelGGL(k_gather_take, dim3(nb), dim3(kGatherThreads), 0, stream, a, take_off, part);
            RK_HIP(ctx, hipGetLastError());
            st->launches += 2;
            total_picks += home.picks;
        }
    }
    // the result in one block, one copy
    const size_t head = Result::head_bytes(Q), bytes = head + total_picks * sizeof(rk_gather_pick);
    DevBuf<unsigned char> block(ctx);
    RK_HIP(ctx, block.alloc(bytes));
    hipLaunchKernelGGL(k_query_scan<kGatherThreads>, dim3(1), dim3(kGatherThreads), 0, stream, per_q.p + 3 * (size_t)Q, (const uint32_t *)nullptr, Q, 0u, (unsigned long long *)block.p,
                       &cnt_dev.p->take_total);
    RK_HIP(ctx, hipGetLastError());
    st->launches++;
    if (Q) RK_HIP(ctx, hipMemcpyAsync(block.p + ((size_t)Q + 1) * 8, per_q.p + Q, (size_t)4 * Q, hipMemcpyDeviceToDevice, stream));              // matched
    if (Q) RK_HIP(ctx, hipMemcpyAsync(block.p + ((size_t)Q + 1) * 8 + (size_t)4 * Q, per_q.p, (size_t)4 * Q, hipMemcpyDeviceToDevice, stream));   // n_cand
    if (Q) RK_HIP(ctx, hipMemcpyAsync(block.p + ((size_t)Q + 1) * 8 + (size_t)8 * Q, per_q.p + 2 * (size_t)Q, (size_t)4 * Q, hipMemcpyDeviceToDevice, stream));
    size_t at = head;
    for (const auto &p : taken.parts) {
        RK_HIP(ctx, hipMemcpyAsync(block.p + at, p.first, p.second * sizeof(rk_gather_pick), hipMemcpyDeviceToDevice, stream));
        at += p.second * sizeof(rk_gather_pick);
    }
    RK_HIP(ctx, span.end());
    res->block.resize(bytes);
    RK_HIP(ctx, hipMemcpyAsync(res->block.data(), block.p, bytes, hipMemcpyDeviceToHost, stream));
    RK_HIP(ctx, hipStreamSynchronize(stream));
    span.read();
    res->n_picks = total_picks;
    const uint64_t *off = (const uint64_t *)res->block.data();
    if (off[0] != 0 || off[Q] != total_picks) return rk_fail(ctx, RK_ERR_HIP, "rk_gather_rows: the offsets of the rows do not span the picks (internal error)");
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_gather_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off, const uint64_t *q_lists, uint32_t n_query,
                    uint32_t n_ref, const uint32_t *ref_sizes, const uint32_t *query_sizes, const rk_gather_opts *opts, uint64_t *off_out,
                    rk_gather_pick **picks_out, uint64_t *n_picks, uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *covered_out)
{
    if (!q_off || !opts || !off_out || !picks_out || !n_picks) return RK_ERR_ARG;
    if (n_query && (!query_sizes || !matched_out || !n_cand_out || !covered_out)) return RK_ERR_ARG;
    if ((n_lists && !counts) || (n_ref && !ref_sizes) || !opts->min_new) return RK_ERR_ARG;
    if (q_off[0] != 0) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        if (q_off[q + 1] < q_off[q]) return RK_ERR_ARG;
    if (q_off[n_query] && !q_lists) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        for (uint64_t j = q_off[q]; j < q_off[q + 1]; j++)
            if (q_lists[j] >= n_lists || (j > q_off[q] && q_lists[j - 1] >= q_lists[j])) return RK_ERR_ARG;
    uint64_t total = 0;
    for (uint64_t u = 0; u < n_lists; u++) total += counts[u];
    if (total && !postings) return RK_ERR_ARG;
    std::vector<uint64_t> pos;
    std::vector<uint32_t> fixed;
    const uint32_t *post = nullptr;
    if (int rc = prepare_lists(postings, counts, n_lists, n_ref, &pos, &fixed, &post)) return rc;
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, n_query);
    HostResult r;
    gather_core(post, pos.data(), q_off, q_lists, n_query, n_ref, ref_sizes, query_sizes, opts, sel, &r);
    return hand_out(view(r), sel, n_query, off_out, picks_out, n_picks, {matched_out, n_cand_out, covered_out});
}

int rk_gather_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_gather_opts *opts, uint64_t *off_out, rk_gather_pick **picks_out,
                   uint64_t *n_picks, uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *covered_out, rk_gather_stats *stats)
{
    if (!ctx || !idx || !queries || !opts || !off_out || !picks_out || !n_picks) return RK_ERR_ARG;
    const char *const who = "rk_gather_rows";
    const uint32_t N = idx->n_ref, Q = queries->n;
    if (Q && (!matched_out || !n_cand_out || !covered_out)) return rk_fail(ctx, RK_ERR_ARG, "%s: matched_out, n_cand_out or covered_out is null", who);
    if (!opts->min_new) return rk_fail(ctx, RK_ERR_ARG, "%s: min_new must be at least 1", who);
    if (queries->wide != idx->wide) return rk_fail(ctx, RK_ERR_ARG, "query sketches and index use different hash widths");
    if (N && (!idx->d_postings || !idx->d_upos || idx->n_shards > 1))
        return rk_fail(ctx, RK_ERR_ARG, "%s: an index without all posting lists (rk_index_join_shard, one hash range of a sharded build)", who);
    if (N && Q && (!idx->ref_sets || !queries->is_set)) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s takes sketches as sets: a sketch repeats a hash", who);
    if (idx->H >= 0x7FFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "explicit queries against an index of 2^31-1 postings or more");
    rk_gather_stats st;
    memset(&st, 0, sizeof st);
    const uint32_t split = rk_switched_off("RK_GATHER_SPLIT") ? 0xFFFFFFFFu : 0u;   // RK_GATHER_SPLIT=0: every list by the lane that found the winner
    const uint32_t lane_max = (uint32_t)std::min<unsigned long long>(env_number("RK_GATHER_LANE_MAX", kLaneMax), 0xFFFFFFFFu);
    fill_constants(&st, split ? split : lane_max, split ? split : std::max(lane_max, kWaveMax), (uint32_t)env_number("RK_GATHER_SYNC_EVERY", kSyncEvery));
    const TimedSpan span{ctx, RK_MS_GATHER};
    span.clear();
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, Q);
    st.rows = (uint32_t)sel.rows.size();
    uint32_t *const outs[3] = {matched_out, n_cand_out, covered_out};
    HostResult host;
    DeviceResult dev;
    Result r;
    const bool runs = N && !sel.rows.empty();   // (else every row is empty: r stays without offsets)
    if (runs && rk_switched_off("RK_GATHER_DEVICE")) {
        st.path = 2;
        RK_TRY(idx->wide ? gather_on_host<uint64_t>(ctx, idx, queries, opts, sel, &host) : gather_on_host<uint32_t>(ctx, idx, queries, opts, sel, &host));
        r = view(host);
        st.batches = 1;
    } else if (runs) {
        st.path = 1;
        RK_TRY(gather_on_device(ctx, idx, queries, opts, sel, &st, &dev));
        r = Result::from_block(dev.block.data(), Q, dev.n_picks);
    }
    if (hand_out(r, sel, Q, off_out, picks_out, n_picks, outs)) return rk_fail(ctx, RK_ERR_NOMEM, "%s: out of host memory", who);
    st.picks = r.n_recs;
    for (const uint32_t q : sel.rows) {
        st.matched += matched_out[q];
        st.candidates += n_cand_out[q];
        st.rounds = std::max<uint32_t>(st.rounds, (uint32_t)(off_out[q + 1] - off_out[q]));
    }
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
