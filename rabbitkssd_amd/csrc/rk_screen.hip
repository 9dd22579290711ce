// rk_screen.hip -- which references are contained in a query sketch, and how much of each survives once every shared hash is credited to
// one reference only (rk_screen_rows): the winner-take-all containment screen of `mash screen -w`, in integers only, and the same rule on
// the host over exported lists (rk_screen_lists).  Sketches are SETS.  Per query with hash set S: matched = the hashes of S with a posting
// list, common(r) = |S n R_r|, the candidates = the references with common >= min_common.  Candidate a is better than b when
// common(a) size(b) > common(b) size(a) (64-bit products, exact: every size is below 2^30), or the products are equal and size(a) > size(b),
// or the sizes are equal too and the CALLER's index of a is smaller.  A matched hash is claimed by the best candidate among its holders;
// won(r) = the hashes r claims.  One record per candidate with won >= min_won, in (query, caller's index) order.  include/rabbitkssd.h,
// winner-take-all containment screen.
//
// Per batch of query rows (as many counter rows and won rows as RK_SCREEN_BATCH_BYTES holds), all on ctx->stream:
//   counts   rk_distq_counts (stage A of rk_dist_topn): int32 cnt[slot][N], columns in the caller's order; won[slot][N] starts at 0;
//   winners  k_screen_win: flat over ALL query hashes of the batch in tiles of kTileHashes, whatever sketch they belong to.  Per hash its
//            slot (a binary search among the batch's hash offsets: runs of empty sketches fall out), the look-up (rk_query_dev.h), then
//            the walk of its posting list by its length: the lane that found it up to lane_max postings, its wave up to wave_max (64
//            postings per trip, a wave reduction of the best key), the workgroup beyond (an LDS queue, partial keys per wave).  Per posting
//            p: r = orig[p], c = cnt[slot][r]; below min_common it is skipped, else (c, size, r) is compared with the best so far.  The
//            winner takes +1 on won[slot][r], a relaxed agent-scope add; equal (slot, winner) of a wave are combined first (up to
//            kCombineRounds leaders by ballots, the rest lane by lane; RK_SCREEN_COMBINE=0: every add lane by lane);
//   count    k_screen_count, one workgroup per row: n_cand = the cells with cnt >= min_common, the records = those with won >= min_won,
//            claimed = the sum of won;
//   scan     k_query_scan (rk_query_dev.h) over the rows' record counts; ONE read-back of the counters gives the room;
//   write    k_screen_write, one workgroup per row, the row in chunks of the block size with a block scan: the records come out by
//            ascending caller's index without atomics and without a sort;
//   result   off[Q + 1] by k_query_scan over all rows; ONE copy to the host: 8 (Q + 1) + 12 Q + 24 records bytes.
//
// rk_screen_abund_rows (counted queries: per record the sum and the lower median of the counts over what it shares and over what it claims)
// runs the same batches with the count and the write kernel in their ABUND instantiation, then the fill and select kernels of
// rk_screen_abund.inc per sub-range of rows; rk_screen_abund_lists is screen_core with q_counts.  DESIGN.md 4.20.
//
// Memory scope: every array is written by one kernel and read by a later one on the same stream.  INSIDE a launch the only communication
// between workgroups is relaxed agent-scope atomic adds -- the +1 on the won rows, matched[] and the statistics, none of which is read
// before the launch is over -- and LDS between barriers.  No loop waits for another workgroup: any grid works.  DESIGN.md 4.18.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rk_internal.h"
#include "rk_query_dev.h"
#include "rk_query_host.h"

namespace {

constexpr int kScreenThreads = 256;                 // threads of every workgroup of this unit: 4 waves
constexpr int kWaves = kScreenThreads / 64;
constexpr uint32_t kLaneMax = 16;                   // the longest list the lane that found it walks itself
constexpr uint32_t kWaveMax = 1024;                 // the longest list its wave walks (64 postings per trip); beyond: the workgroup
constexpr int kTrips = 4;                           // runs of 64 hashes one wave takes of a tile
constexpr int kTileHashes = kScreenThreads * kTrips;   // 1024
constexpr int kCombineRounds = 4;                   // leaders of a wave whose equal (slot, winner) are added once
constexpr uint32_t kSizeLimit = 1u << 30;           // sizes at or above it are refused: common * size stays below 2^60
static_assert(sizeof(rk_screen_opts) == 20 && sizeof(rk_screen_rec) == 24 && sizeof(rk_screen_stats) == 120, "the layouts of include/rabbitkssd.h");
static_assert(kLaneMax < kWaveMax && kWaveMax % 64 == 0, "the classes of list lengths");

struct Counters {   // one device block, read back in one copy
    unsigned long long walked, adds, lane_lists, wave_lists, block_lists, rec_total, all_total;
};

// (common, size, caller's index) of a candidate; c == 0: none
struct Key {
    uint32_t c, sz, r;
};

// the order of the candidates of a row: include/rabbitkssd.h.  Both products lie below 2^60.
__host__ __device__ __forceinline__ bool better(const Key &a, const Key &b)
{
    if (!a.c) return false;
    if (!b.c) return true;
    const unsigned long long ab = (unsigned long long)a.c * b.sz, ba = (unsigned long long)b.c * a.sz;
    if (ab != ba) return ab > ba;
    if (a.sz != b.sz) return a.sz > b.sz;
    return a.r < b.r;
}

// the best key of a wave, in every lane (the order is total: every lane ends with the same key)
__device__ __forceinline__ Key wave_best(Key k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Key x;
        x.c = (uint32_t)__shfl_xor((int)k.c, o);
        x.sz = (uint32_t)__shfl_xor((int)k.sz, o);
        x.r = (uint32_t)__shfl_xor((int)k.r, o);
        if (better(x, k)) k = x;
    }
    return k;
}

struct WinArgs {
    const void *q_hashes;              // Hash[total]
    const uint64_t *q_off;             // u64[Q + 1]
    const uint32_t *row_of;            // the batch: slot s is query row row_of[s]
    const unsigned long long *hoff;    // nb + 1: the hashes of the slots before s, from hoff[0] (any base)
    uint32_t nb;
    unsigned long long n_hashes;       // hoff[nb] - hoff[0]
    IndexLookup ix;
    const uint32_t *postings, *upos, *orig, *sizes_internal;   // the index (orig null: the identity)
    const int32_t *cnt;                // [nb][n_ref], columns in the caller's order
    uint32_t *won;                     // [nb][n_ref]
    uint32_t n_ref, min_common, lane_max, wave_max;
    uint32_t *matched_q;               // per QUERY row
    Counters *c;
};

struct Walk {   // what one walk reads
    const uint32_t *postings, *orig, *sizes_internal;
    const int32_t *cnt;
    uint32_t min_common;
    __device__ __forceinline__ void see(uint32_t at, Key *best) const
    {
        const uint32_t p = postings[at];
        Key k;
        k.r = orig ? orig[p] : p;           // (p < n_ref and orig[] < n_ref: the index's own arrays)
        k.c = (uint32_t)cnt[k.r];
        if (k.c < min_common) return;       // (min_common >= 1)
        k.sz = sizes_internal[p];
        if (better(k, *best)) *best = k;
    }
};

template <class Hash, bool COMBINE> __global__ void __launch_bounds__(kScreenThreads) k_screen_win(WinArgs a)
{
    __shared__ uint32_t s_qn[kTrips], s_qbeg[kScreenThreads], s_qlen[kScreenThreads], s_qslot[kScreenThreads];
    __shared__ Key s_part[kScreenThreads][kWaves];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < (uint32_t)kTrips) s_qn[tid] = 0;   // one counter per trip: none is reset while another wave may still read it
    const unsigned long long base = (unsigned long long)blockIdx.x * kTileHashes + (unsigned long long)wave * (kTrips * 64);
    const Hash *q = (const Hash *)a.q_hashes;
    const unsigned long long h0 = a.hoff[0];
    // the slot of hash j of the batch: the last s with hoff[s] - h0 <= j (j < n_hashes: s < nb); the searches of a lane advance together
    uint32_t slo[kTrips], shi[kTrips];
    bool in[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        in[t] = base + 64 * t + lane < a.n_hashes;
        slo[t] = 0;
        shi[t] = in[t] ? a.nb - 1 : 0u;
    }
    for (bool more = true; more;) {
        more = false;
#pragma unroll
        for (int t = 0; t < kTrips; t++)
            if (slo[t] < shi[t]) {
                const uint32_t mid = slo[t] + (shi[t] - slo[t] + 1) / 2;   // (1 <= mid <= nb - 1)
                if (a.hoff[mid] - h0 <= base + 64 * t + lane) slo[t] = mid; else shi[t] = mid - 1;
                more |= slo[t] < shi[t];
            }
    }
    unsigned long long h[kTrips];
    uint32_t list[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        h[t] = 0;
        if (in[t]) {
            const uint32_t row = a.row_of[slo[t]];
            h[t] = (unsigned long long)q[a.q_off[row] + (base + 64 * t + lane - (a.hoff[slo[t]] - h0))];
        }
    }
    index_lookup<Hash, kTrips>(a.ix, h, in, list);
    unsigned long long walked = 0, adds = 0, n_lane = 0, n_wave = 0, n_block = 0;
    __syncthreads();   // (s_qn)
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const uint32_t slot = slo[t];
        uint32_t beg = 0, len = 0;
        if (list[t] != kNoList) {
            beg = a.upos[list[t]];
            len = a.upos[list[t] + 1] - beg;
        }
        const bool found = len > 0;
        // matched: the equal slots of a run of 64 hashes are counted by ballots (neighbours share their row), one add per slot and wave
        {
            unsigned long long pending = __ballot(found);
            while (pending) {   // (uniform)
                const int lead = __ffsll((long long)pending) - 1;
                const uint32_t sl = (uint32_t)__shfl((int)slot, lead);
                const unsigned long long m = __ballot(found && slot == sl);
                if (lane == lead) add_u32(a.matched_q + a.row_of[sl], (uint32_t)__popcll(m));
                pending &= ~m;
            }
        }
        const bool by_lane = found && len <= a.lane_max, by_wave = found && !by_lane && len <= a.wave_max, by_block = found && !by_lane && !by_wave;
        Walk wk{a.postings, a.orig, a.sizes_internal, a.cnt + (size_t)slot * a.n_ref, a.min_common};
        Key win{0, 0, 0};
        if (by_lane)
            for (uint32_t j = 0; j < len; j++) wk.see(beg + j, &win);
        unsigned long long pending = __ballot(by_wave);
        while (pending) {   // (uniform in the wave)
            const int src = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t b = (uint32_t)__shfl((int)beg, src), l = (uint32_t)__shfl((int)len, src), sl = (uint32_t)__shfl((int)slot, src);
            Walk ww{a.postings, a.orig, a.sizes_internal, a.cnt + (size_t)sl * a.n_ref, a.min_common};
            Key mine{0, 0, 0};
            for (uint32_t j = lane; j < l; j += 64) ww.see(b + j, &mine);
            mine = wave_best(mine);
            if (lane == src) win = mine;
        }
        uint32_t at = 0;
        if (by_block) {
            at = atomicAdd(&s_qn[t], 1u);   // (at most one per thread and trip: at < kScreenThreads)
            s_qbeg[at] = beg;
            s_qlen[at] = len;
            s_qslot[at] = slot;
        }
        __syncthreads();
        const uint32_t qn = s_qn[t];
        if (qn) {   // (uniform in the workgroup)
            for (uint32_t k = 0; k < qn; k++) {
                Walk wb{a.postings, a.orig, a.sizes_internal, a.cnt + (size_t)s_qslot[k] * a.n_ref, a.min_common};
                const uint32_t b = s_qbeg[k], l = s_qlen[k];
                Key mine{0, 0, 0};
                for (uint32_t j = tid; j < l; j += kScreenThreads) wb.see(b + j, &mine);
                mine = wave_best(mine);
                if (lane == 0) s_part[k][wave] = mine;
            }
            __syncthreads();
            if (by_block) {
                win = s_part[at][0];
#pragma unroll
                for (int w = 1; w < kWaves; w++)
                    if (better(s_part[at][w], win)) win = s_part[at][w];
            }
            __syncthreads();   // (the queue and the partial keys are free for the next trip)
        }
        // the winners' +1: won[slot][r]
        bool has = win.c != 0;
        const unsigned long long key = ((unsigned long long)slot << 32) | win.r;
        if (COMBINE) {
            unsigned long long todo = __ballot(has);
            for (int round = 0; round < kCombineRounds && todo; round++) {   // (uniform)
                const int lead = __ffsll((long long)todo) - 1;
                const unsigned long long kl = shfl_u64(key, lead);
                const bool same = has && key == kl;
                const unsigned long long m = __ballot(same);
                if (lane == lead) {
                    add_u32(a.won + (size_t)slot * a.n_ref + win.r, (uint32_t)__popcll(m));
                    adds++;
                }
                if (same) has = false;
                todo &= ~m;
            }
        }
        if (has) {
            add_u32(a.won + (size_t)slot * a.n_ref + win.r, 1u);
            adds++;
        }
        walked += len;
        n_lane += by_lane;
        n_wave += by_wave;
        n_block += by_block;
    }
    // the statistics: one atomic per wave and counter that moved
    walked = wave_sum(walked);
    adds = wave_sum(adds);
    n_lane = wave_sum(n_lane);
    n_wave = wave_sum(n_wave);
    n_block = wave_sum(n_block);
    if (lane == 0) {
        if (walked) add_u64(&a.c->walked, walked);
        if (adds) add_u64(&a.c->adds, adds);
        if (n_lane) add_u64(&a.c->lane_lists, n_lane);
        if (n_wave) add_u64(&a.c->wave_lists, n_wave);
        if (n_block) add_u64(&a.c->block_lists, n_block);
    }
}

struct RowArgs {   // a batch of nb rows: slot s of the batch is query row row_of[s], its rows cnt + s * n_ref and won + s * n_ref
    const int32_t *cnt;
    const uint32_t *won;
    const uint32_t *row_of;
    uint32_t n_ref, min_common, min_won;
    uint32_t *n_cand_q, *claimed_q, *nrec_q;   // per QUERY row
    const unsigned long long *rec_off;         // per slot: nb + 1
    rk_screen_rec *recs;
    const uint32_t *sizes;                     // per caller's reference index
    const uint64_t *q_off;
    // ABUND only (rk_screen_abund.inc): per slot the records of the row, the sum and the largest of their common, for the batch's one read-back;
    // per slot where the row's values begin; the won rows once more, as the map; per record where its values begin
    unsigned long long *row_recs, *row_vals, *row_longest;
    const unsigned long long *val_off;
    uint32_t *map;
    unsigned long long *seg;
};

// One workgroup per row: the candidates, the records and the sum of won; ABUND: also the sum and the largest of common over the records
template <bool ABUND> __global__ void __launch_bounds__(kScreenThreads) k_screen_count(RowArgs a)
{
    __shared__ uint32_t s_cand, s_rec, s_claimed;
    [[maybe_unused]] __shared__ unsigned long long s_vals;
    [[maybe_unused]] __shared__ uint32_t s_longest;
    [[maybe_unused]] unsigned long long vals = 0;
    [[maybe_unused]] uint32_t longest = 0;
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const int32_t *cnt = a.cnt + (size_t)s * a.n_ref;
    const uint32_t *won = a.won + (size_t)s * a.n_ref;
    if (tid == 0) s_cand = s_rec = s_claimed = 0;
    if constexpr (ABUND)
        if (tid == 0) {
            s_vals = 0;
            s_longest = 0;
        }
    __syncthreads();
    uint32_t n_cand = 0, n_rec = 0, claimed = 0;
    for (uint32_t c = tid; c < a.n_ref; c += kScreenThreads) {
        const bool cand = (uint32_t)cnt[c] >= a.min_common;
        const uint32_t w = won[c];   // (only a candidate wins)
        n_cand += cand;
        n_rec += cand && w >= a.min_won;
        claimed += w;
        if constexpr (ABUND)
            if (cand && w >= a.min_won) {
                vals += (uint32_t)cnt[c];
                longest = max(longest, (uint32_t)cnt[c]);
            }
    }
    if (n_cand) atomicAdd(&s_cand, n_cand);
    if (n_rec) atomicAdd(&s_rec, n_rec);
    if (claimed) atomicAdd(&s_claimed, claimed);
    if constexpr (ABUND)
        if (vals) {
            atomicAdd(&s_vals, vals);
            atomicMax(&s_longest, longest);
        }
    __syncthreads();
    if (tid == 0) {
        const uint32_t row = a.row_of[s];
        a.n_cand_q[row] = s_cand;
        a.nrec_q[row] = s_rec;
        a.claimed_q[row] = s_claimed;
        if constexpr (ABUND) {
            a.row_recs[s] = s_rec;
            a.row_vals[s] = s_vals;
            a.row_longest[s] = s_longest;
        }
    }
}

// One workgroup per row, the row in chunks of the block size: the records at rec_off[s] + the records of the cells before, in the
// order of the cells.  ABUND: also map[cell] = the record of the cell + 1 (0: none) over the won row, which nobody reads again, and
// seg[record] = val_off[s] + the common of the row's records before it
template <bool ABUND> __global__ void __launch_bounds__(kScreenThreads) k_screen_write(RowArgs a)
{
    __shared__ uint32_t s_cnt[kWaves];
    [[maybe_unused]] __shared__ unsigned long long s_val[kWaves];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int32_t *cnt = a.cnt + (size_t)s * a.n_ref;
    const uint32_t *won = a.won + (size_t)s * a.n_ref;
    const unsigned long long beg = a.rec_off[s], room = a.rec_off[s + 1] - beg;
    if (!room) {   // (uniform)
        if constexpr (ABUND)
            for (uint32_t c = tid; c < a.n_ref; c += kScreenThreads) a.map[(size_t)s * a.n_ref + c] = 0;
        return;
    }
    const uint32_t row = a.row_of[s], size_query = (uint32_t)(a.q_off[row + 1] - a.q_off[row]);
    unsigned long long run = 0;
    [[maybe_unused]] unsigned long long vrun = 0, vincl = 0;
    if constexpr (ABUND) vrun = a.val_off[s];
    for (uint32_t c0 = 0; c0 < a.n_ref; c0 += kScreenThreads) {   // (uniform)
        const uint32_t c = c0 + tid;
        uint32_t common = 0, wn = 0;
        bool keep = false;
        if (c < a.n_ref) {
            common = (uint32_t)cnt[c];
            wn = won[c];
            keep = common >= a.min_common && wn >= a.min_won;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[w] = (uint32_t)__popcll(m);
        if constexpr (ABUND) {   // the common of the kept cells up to and with this lane's
            vincl = keep ? common : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long x = shfl_u64(vincl, (lane - o) & 63);
                if (lane >= o) vincl += x;
            }
            if (lane == 63) s_val[w] = vincl;
        }
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            if (k < w) before += s_cnt[k];
            all += s_cnt[k];
        }
        const unsigned long long at = run + before + (uint32_t)__popcll(m & lanes_below(lane));
        if (keep && at < room) a.recs[beg + at] = rk_screen_rec{row, c, common, wn, a.sizes[c], size_query};
        if constexpr (ABUND) {
            unsigned long long vbefore = 0, vall = 0;
#pragma unroll
            for (int k = 0; k < kWaves; k++) {
                if (k < w) vbefore += s_val[k];
                vall += s_val[k];
            }
            if (keep && at < room) a.seg[beg + at] = vrun + vbefore + vincl - common;
            if (c < a.n_ref) a.map[(size_t)s * a.n_ref + c] = keep && at < room ? (uint32_t)(beg + at + 1) : 0u;
            vrun += vall;
        }
        run += all;
        __syncthreads();   // (s_cnt is rewritten by the next chunk)
    }
}

#include "rk_screen_abund.inc"

// ---- host: the rule, exactly ------------------------------------------------------------------------------------------------
struct HostResult {
    std::vector<rk_screen_rec> recs;
    std::vector<uint64_t> off;                          // Q + 1
    std::vector<uint32_t> matched, n_cand, claimed;     // Q (unselected rows: 0)
    uint64_t walked = 0, lane_lists = 0, wave_lists = 0, block_lists = 0;
    // with q_counts only: one per record; per row the sums of the counts over the matched and over the claimed hashes at 3 q + 1, 3 q + 2
    std::vector<rk_screen_abund> abund;
    std::vector<uint64_t> occ;
    uint64_t values = 0, rank_segs = 0, wave_segs = 0, block_segs = 0;
};

// the sum and the lower median of v[0 .. n), n > 0 (v is reordered)
void sum_and_median(uint32_t *v, size_t n, uint64_t *sum, uint32_t *med)
{
    uint64_t s = 0;
    for (size_t i = 0; i < n; i++) s += v[i];
    std::nth_element(v, v + (n - 1) / 2, v + n);
    *sum = s;
    *med = v[(n - 1) / 2];
}

// lists: list u is post[pos[u] .. pos[u + 1]), strictly ascending reference ids below n_ref.  The winner of a list is found by scanning
// its candidates with the comparator -- no ranking of the row, unlike tests/_screen_ref.py's second statement.
// RK_ERR_ARG (strict only): a reference of a selected row shares more hashes than its size.
// q_counts (parallel to q_lists; null: the plain screen): the abundance records, as rk_screen_abund.inc lays them out -- every holder with
// a record takes the count of the hash, the winner's from the front of its segment, everybody else's from the back.
int screen_core(const uint32_t *post, const uint64_t *pos, const uint64_t *q_off, const uint64_t *q_lists, const uint32_t *q_counts, uint32_t Q, uint32_t n_ref,
                const uint32_t *ref_sizes, const uint32_t *query_sizes, const rk_screen_opts *o, const RowSel &sel, bool strict, HostResult *out)
{
    std::vector<uint32_t> common(n_ref, 0), won(n_ref, 0), touched, n_rec(Q, 0);
    std::vector<uint32_t> winner, vals, front, back;
    std::vector<uint64_t> seg;
    if (q_counts) {
        out->occ.assign((size_t)3 * Q, 0);
        seg.assign(n_ref, 0);
        front.assign(n_ref, 0);
        back.assign(n_ref, 0);
    }
    out->matched.assign(Q, 0);
    out->n_cand.assign(Q, 0);
    out->claimed.assign(Q, 0);
    for (const uint32_t q : sel.rows) {
        const uint64_t *lists = q_lists + q_off[q];
        const uint64_t nl = q_off[q + 1] - q_off[q];
        touched.clear();
        uint32_t matched = 0;
        for (uint64_t k = 0; k < nl; k++) {
            const uint64_t u = lists[k], len = pos[u + 1] - pos[u];
            matched += len > 0;   // (an empty list matches nothing)
            for (uint64_t i = pos[u]; i < pos[u + 1]; i++)
                if (!common[post[i]]++) touched.push_back(post[i]);
            out->walked += len;
            if (len && len <= kLaneMax) out->lane_lists++;
            else if (len && len <= kWaveMax) out->wave_lists++;
            else if (len) out->block_lists++;
        }
        bool bad = false;
        for (const uint32_t r : touched) bad = bad || (strict && common[r] > ref_sizes[r]);
        if (bad) return RK_ERR_ARG;
        uint32_t claimed = 0;
        if (q_counts) winner.assign(nl, UINT32_MAX);
        for (uint64_t k = 0; k < nl; k++) {
            Key best{0, 0, 0};
            for (uint64_t i = pos[lists[k]]; i < pos[lists[k] + 1]; i++) {
                const uint32_t r = post[i];
                const Key key{common[r], ref_sizes[r], r};
                if (key.c >= o->min_common && better(key, best)) best = key;
            }
            if (best.c) {
                won[best.r]++;
                claimed++;
                if (q_counts) {
                    winner[k] = best.r;
                    out->occ[(size_t)3 * q + 2] += q_counts[q_off[q] + k];
                }
            }
            if (q_counts && pos[lists[k] + 1] > pos[lists[k]]) out->occ[(size_t)3 * q + 1] += q_counts[q_off[q] + k];
        }
        std::sort(touched.begin(), touched.end());
        if (q_counts) {   // the segments of the records, then the values
            uint64_t room = 0;
            for (const uint32_t r : touched)
                if (common[r] >= o->min_common && won[r] >= o->min_won) {
                    seg[r] = room;
                    room += common[r];
                }
            vals.assign(room, 0);
            for (uint64_t k = 0; k < nl; k++)
                for (uint64_t i = pos[lists[k]]; i < pos[lists[k] + 1]; i++) {
                    const uint32_t r = post[i];
                    if (common[r] < o->min_common || won[r] < o->min_won) continue;
                    vals[seg[r] + (winner[k] == r ? front[r]++ : common[r] - 1 - back[r]++)] = q_counts[q_off[q] + k];
                }
            out->values += room;
        }
        uint32_t n_cand = 0;
        for (const uint32_t r : touched) {
            if (common[r] >= o->min_common) {
                n_cand++;
                if (won[r] >= o->min_won) {
                    out->recs.push_back(rk_screen_rec{q, r, common[r], won[r], ref_sizes[r], query_sizes[q]});
                    n_rec[q]++;
                    if (q_counts) {
                        rk_screen_abund ab{0, 0, 0, 0};
                        if (won[r]) sum_and_median(vals.data() + seg[r], won[r], &ab.occ_won, &ab.med_won);
                        sum_and_median(vals.data() + seg[r], common[r], &ab.occ_common, &ab.med_common);
                        out->abund.push_back(ab);
                        if (common[r] <= kRankMax) out->rank_segs++;
                        else if (common[r] <= kWaveSelMax) out->wave_segs++;
                        else out->block_segs++;
                    }
                }
                if (q_counts) front[r] = back[r] = 0;
            }
            common[r] = won[r] = 0;
        }
        out->matched[q] = matched;
        out->n_cand[q] = n_cand;
        out->claimed[q] = claimed;
    }
    out->off.assign((size_t)Q + 1, 0);
    for (uint32_t q = 0; q < Q; q++) out->off[q + 1] = out->off[q] + n_rec[q];
    return RK_OK;
}

using Result = RowsResult<rk_screen_rec, 3>;   // per row: matched, n_cand, claimed

Result view(const HostResult &r)
{
    return Result{r.off.data(), {r.matched.data(), r.n_cand.data(), r.claimed.data()}, r.recs.data(), r.recs.size()};
}

void fill_constants(rk_screen_stats *st)
{
    st->lane_max = kLaneMax;
    st->wave_max = kWaveMax;
    st->tile_hashes = kTileHashes;
    st->threads = kScreenThreads;
}

unsigned long long env_number(const char *name, unsigned long long otherwise)
{
    const char *sw = getenv(name);
    const unsigned long long v = sw ? strtoull(sw, nullptr, 10) : 0;
    return v ? v : otherwise;
}

// RK_SCREEN_DEVICE=0: export + the lists of the selected queries' hashes (a binary search each) + the rule on the host
// (abund: the counts of the queries go along, rk_screen_abund_rows)
template <class Hash> int screen_on_host(rk_ctx *ctx, const rk_index *idx, const rk_sketches *qs, const rk_screen_opts *o, const RowSel &sel, bool abund, HostResult *out)
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
    std::vector<uint64_t> l_off((size_t)Q + 1, 0), l, whole((size_t)(abund ? Q : 0), 0);
    std::vector<uint32_t> qc((size_t)(abund ? qs->total : 0)), lc;
    if (abund) RK_TRY(rk_sketches_download_counts(qs, qc.data()));
    size_t next = 0;
    for (uint32_t q = 0; q < Q; q++) {
        query_sizes[q] = (uint32_t)(qoff[q + 1] - qoff[q]);
        if (next < sel.rows.size() && sel.rows[next] == q) {
            next++;
            for (uint64_t j = qoff[q]; j < qoff[q + 1]; j++) {
                const auto it = std::lower_bound(hashes.begin(), hashes.end(), qh[j]);
                if (it != hashes.end() && *it == qh[j]) {
                    l.push_back((uint64_t)(it - hashes.begin()));
                    if (abund) lc.push_back(qc[j]);
                }
                if (abund) whole[q] += qc[j];
            }
        }
        l_off[q + 1] = l.size();
    }
    std::vector<uint64_t> pos;
    std::vector<uint32_t> fixed;
    const uint32_t *post = nullptr;
    if (prepare_lists(postings.data(), counts.data(), idx->U, N, &pos, &fixed, &post))
        return rk_fail(ctx, RK_ERR_HIP, "rk_screen_rows: an exported posting names a genome beyond their number (internal error)");
    static const uint32_t none = 0;   // (abund without a hit: q_counts must not be null)
    RK_TRY(screen_core(post, pos.data(), l_off.data(), l.data(), abund ? (lc.empty() ? &none : lc.data()) : nullptr, Q, N, ref_sizes.data(), query_sizes.data(), o, sel,
                       false, out));
    for (uint32_t q = 0; abund && q < Q; q++) out->occ[(size_t)3 * q] = whole[q];
    return RK_OK;
}

struct DeviceResult {
    std::vector<unsigned char> block;   // Result::from_block
    uint64_t n_recs = 0;
};

constexpr unsigned long long kSelectRecs = 1ULL << 30;   // the records one launch of a select kernel takes

struct AbundDevice {   // what rk_screen_abund_rows adds to the device leg
    std::vector<unsigned char> block;   // rk_screen_abund[n_recs] | u64 occ[3 Q] | AbundCounters
    uint64_t values = 0, value_bytes = 0;
    uint32_t passes = 0;
};

// ab != null: rk_screen_abund_rows (the queries carry counts)
int screen_on_device(rk_ctx *ctx, const rk_index *idx, const rk_sketches *qs, const rk_screen_opts *o, const RowSel &sel, rk_screen_stats *st, DeviceResult *res,
                     AbundDevice *ab)
{
    const uint32_t N = idx->n_ref, Q = qs->n;
    const uint64_t n_sel = sel.rows.size();
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const TimedSpan span{ctx, ab ? RK_MS_SCREEN_ABUND : RK_MS_SCREEN};
    const bool combine = !rk_switched_off("RK_SCREEN_COMBINE");
    RK_TRY(rk_index_ensure_dir(ctx, const_cast<rk_index *>(idx), stream));
    rk_dist_opts dopts;   // the row shard for rk_distq_counts; nothing of a distance is evaluated
    memset(&dopts, 0, sizeof dopts);
    dopts.kmer_size = 1;
    dopts.max_dist = 1.0;
    dopts.row_block = (int32_t)std::min<uint32_t>(o->row_block, (uint32_t)INT_MAX);
    dopts.row_first = o->row_first;
    dopts.row_step = o->row_step;

    // the selected rows and the hashes before each of them, uploaded once (pageable memory of this function: the stream is synchronised
    // by the first read-back, before the vectors go)
    std::vector<unsigned long long> hoff(n_sel + 1, 0);
    for (uint64_t s = 0; s < n_sel; s++) hoff[s + 1] = hoff[s] + (qs->h_off[sel.rows[s] + 1] - qs->h_off[sel.rows[s]]);

    DevBuf<uint32_t> per_q(ctx), sizes(ctx), row_of(ctx), won(ctx);
    DevBuf<Counters> cnt_dev(ctx);
    DevBuf<unsigned long long> hoff_dev(ctx), rec_off(ctx);
    DevBuf<int32_t> counts(ctx);
    RK_HIP(ctx, per_q.alloc((size_t)4 * Q));   // n_cand, matched, claimed, nrec
    RK_HIP(ctx, sizes.alloc(N));
    RK_HIP(ctx, cnt_dev.alloc(1));
    RK_HIP(ctx, row_of.alloc(n_sel));
    RK_HIP(ctx, hoff_dev.alloc(n_sel + 1));
    RK_HIP(ctx, hipMemsetAsync(per_q.p, 0, (size_t)16 * Q, stream));
    RK_HIP(ctx, hipMemcpyAsync(row_of.p, sel.rows.data(), (size_t)n_sel * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemcpyAsync(hoff_dev.p, hoff.data(), (size_t)(n_sel + 1) * 8, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, span.begin());
    hipLaunchKernelGGL(k_query_prepare, dim3(blocks_for(N)), dim3(kThreads), 0, stream, idx->relabeled ? idx->d_orig : nullptr, idx->d_sizes, N, (uint32_t *)nullptr,
                       sizes.p);
    RK_HIP(ctx, hipGetLastError());
    st->launches++;

    // device bytes of one row of a batch: its counter row and its won row
    const uint64_t row_bytes = (uint64_t)N * 8 + 16;
    const uint64_t batch_bytes = env_number("RK_SCREEN_BATCH_BYTES", 1ULL << 30);
    uint64_t rows_per_batch = std::max<uint64_t>(1, std::min<uint64_t>(n_sel, batch_bytes / row_bytes));
    if (ab) rows_per_batch = std::min<uint64_t>(rows_per_batch, std::max<uint64_t>(1, 0xFFFFFFFEULL / N));   // a record of a batch + 1 fits 32 bits
    st->rows_per_batch = rows_per_batch;
    RK_HIP(ctx, counts.alloc(rows_per_batch * N));
    RK_HIP(ctx, won.alloc(rows_per_batch * N));
    RK_HIP(ctx, rec_off.alloc(rows_per_batch + 1));
    // ab: the counters of a batch, the records of its rows and the sums of their common in ONE block: one read-back
    Counters *cnt = cnt_dev.p;
    DevBuf<unsigned char> home_dev(ctx);
    DevBuf<unsigned long long> val_off(ctx), occ_dev(ctx);
    DevBuf<AbundCounters> abc_dev(ctx);
    std::vector<unsigned char> home_host;
    std::vector<std::vector<unsigned long long>> uploads;   // pageable sources of copies: alive until the last synchronisation
    const size_t home_bytes = sizeof(Counters) + (ab ? (size_t)24 * rows_per_batch : 0);
    if (ab) {
        RK_HIP(ctx, home_dev.alloc(home_bytes));
        cnt = (Counters *)home_dev.p;
        home_host.resize(home_bytes);
        RK_HIP(ctx, val_off.alloc(rows_per_batch));
        RK_HIP(ctx, occ_dev.alloc((size_t)3 * Q));
        RK_HIP(ctx, abc_dev.alloc(1));
        RK_HIP(ctx, hipMemsetAsync(occ_dev.p, 0, (size_t)24 * Q, stream));
        RK_HIP(ctx, hipMemsetAsync(abc_dev.p, 0, sizeof(AbundCounters), stream));
        ab->value_bytes = env_number("RK_SCREEN_VALUE_BYTES", batch_bytes);
    }
    unsigned long long *const row_recs = ab ? (unsigned long long *)(home_dev.p + sizeof(Counters)) : nullptr, *const row_vals = ab ? row_recs + rows_per_batch : nullptr,
                       *const row_longest = ab ? row_vals + rows_per_batch : nullptr;
    struct TakenAbund {   // the abundance records of one batch, as `taken` below
        rk_ctx *ctx;
        std::vector<std::pair<rk_screen_abund *, uint64_t>> parts;
        ~TakenAbund() { for (auto &p : parts) rk_pool_free(ctx, p.first); }
    } taken_abund{ctx, {}};

    struct Taken {   // the records of one batch, in order, until the result is put together
        rk_ctx *ctx;
        std::vector<std::pair<rk_screen_rec *, uint64_t>> parts;
        ~Taken() { for (auto &p : parts) rk_pool_free(ctx, p.first); }
    } taken{ctx, {}};
    uint64_t total_recs = 0;

    for (uint64_t s0 = 0; s0 < n_sel; s0 += rows_per_batch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(rows_per_batch, n_sel - s0);
        st->batches++;
        const uint64_t hashes = hoff[s0 + nb] - hoff[s0], tiles = (hashes + kTileHashes - 1) / kTileHashes;
        if (tiles > 0x7FFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_screen_rows: more than 2^31 tiles of query hashes in one batch");
        RK_TRY(rk_distq_counts(ctx, idx, qs, &dopts, (uint32_t)s0, nb, counts.p, stream));
        RK_HIP(ctx, hipMemsetAsync(won.p, 0, (size_t)nb * N * 4, stream));
        RK_HIP(ctx, hipMemsetAsync(cnt, 0, home_bytes, stream));
        if (tiles && idx->U) {
            WinArgs w;
            memset(&w, 0, sizeof w);
            w.q_hashes = qs->wide ? (const void *)qs->d_hashes64 : (const void *)qs->d_hashes;
            w.q_off = qs->d_off;
            w.row_of = row_of.p + s0;
            w.hoff = hoff_dev.p + s0;
            w.nb = nb;
            w.n_hashes = hashes;
            w.ix = index_lookup_of(idx);
            w.postings = idx->d_postings;
            w.upos = idx->d_upos;
            w.orig = idx->relabeled ? idx->d_orig : nullptr;
            w.sizes_internal = idx->d_sizes;
            w.cnt = counts.p;
            w.won = won.p;
            w.n_ref = N;
            w.min_common = o->min_common;
            w.lane_max = st->lane_max;
            w.wave_max = st->wave_max;
            w.matched_q = per_q.p + Q;
            w.c = cnt;
            const auto win = qs->wide ? (combine ? k_screen_win<uint64_t, true> : k_screen_win<uint64_t, false>)
                                      : (combine ? k_screen_win<uint32_t, true> : k_screen_win<uint32_t, false>);
            hipLaunchKernelGGL(win, dim3((unsigned)tiles), dim3(kScreenThreads), 0, stream, w);
            RK_HIP(ctx, hipGetLastError());
            st->launches++;
        }
        RowArgs a;
        memset(&a, 0, sizeof a);
        a.cnt = counts.p;
        a.won = won.p;
        a.row_of = row_of.p + s0;
        a.n_ref = N;
        a.min_common = o->min_common;
        a.min_won = o->min_won;
        a.n_cand_q = per_q.p;
        a.claimed_q = per_q.p + 2 * (size_t)Q;
        a.nrec_q = per_q.p + 3 * (size_t)Q;
        a.rec_off = rec_off.p;
        a.sizes = sizes.p;
        a.q_off = qs->d_off;
        a.row_recs = row_recs;
        a.row_vals = row_vals;
        a.row_longest = row_longest;
        a.val_off = val_off.p;
        a.map = won.p;
        hipLaunchKernelGGL(ab ? k_screen_count<true> : k_screen_count<false>, dim3(nb), dim3(kScreenThreads), 0, stream, a);
        hipLaunchKernelGGL(k_query_scan<kScreenThreads>, dim3(1), dim3(kScreenThreads), 0, stream, a.nrec_q, a.row_of, nb, 0u, rec_off.p, &cnt->rec_total);
        RK_HIP(ctx, hipGetLastError());
        st->launches += 2;
        Counters home;
        if (ab) {
            RK_TRY(rk_read_back(ctx, home_host.data(), cnt, home_bytes, stream));   // the room of the records and of the values, row by row
            memcpy(&home, home_host.data(), sizeof home);
        } else {
            RK_TRY(rk_read_back(ctx, &home, cnt, sizeof home, stream));   // the room of the records
        }
        st->read_backs++;
        if (home.rec_total > (unsigned long long)nb * N) return rk_fail(ctx, RK_ERR_HIP, "rk_screen_rows: more records than cells (internal error)");
        st->postings_walked += home.walked;
        st->adds += home.adds;
        st->lane_lists += home.lane_lists;
        st->wave_lists += home.wave_lists;
        st->block_lists += home.block_lists;
        if (home.rec_total) {
            rk_screen_rec *part = static_cast<rk_screen_rec *>(rk_pool_alloc(ctx, home.rec_total * sizeof(rk_screen_rec)));
            if (!part) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu records on the device", home.rec_total);
            taken.parts.emplace_back(part, home.rec_total);
            a.recs = part;
            if (!ab) {
                hipLaunchKernelGGL(k_screen_write<false>, dim3(nb), dim3(kScreenThreads), 0, stream, a);
                RK_HIP(ctx, hipGetLastError());
                st->launches++;
            }
            total_recs += home.rec_total;
        }
        if (!ab) continue;
        // ---- the abundances of the batch (rk_screen_abund.inc) ----
        const unsigned long long *recs_h = (const unsigned long long *)(home_host.data() + sizeof(Counters)), *vals_h = recs_h + rows_per_batch,
                                 *longest_h = vals_h + rows_per_batch;
        // the sub-ranges of rows whose values fit the budget, at least one row each; val_off[s]: the values of its sub-range before row s
        std::vector<unsigned long long> voff(nb), rec_before((size_t)nb + 1, 0);
        std::vector<uint32_t> cut{0};   // sub-range k: slots cut[k] .. cut[k + 1]
        unsigned long long run = 0, most = 0, batch_vals = 0;
        for (uint32_t s = 0; s < nb; s++) {
            if (s > cut.back() && (run + vals_h[s]) * 4 > ab->value_bytes) {
                cut.push_back(s);
                run = 0;
            }
            voff[s] = run;
            run += vals_h[s];
            most = std::max(most, run);
            batch_vals += vals_h[s];
            rec_before[s + 1] = rec_before[s] + recs_h[s];
        }
        cut.push_back(nb);
        if (rec_before[nb] != home.rec_total) return rk_fail(ctx, RK_ERR_HIP, "rk_screen_abund_rows: the records of the rows do not add up (internal error)");
        ab->values += batch_vals;
        uploads.push_back(std::move(voff));
        RK_HIP(ctx, hipMemcpyAsync(val_off.p, uploads.back().data(), (size_t)nb * 8, hipMemcpyHostToDevice, stream));
        // (of this batch only: they go back to the pool at the end of the iteration while the kernels that use them may still be queued --
        // safe because everything of this call is on ctx->stream, which orders any reuse of the memory behind them, as DevBuf requires)
        DevBuf<unsigned long long> seg(ctx);
        DevBuf<uint32_t> cur(ctx), vals(ctx);
        RK_HIP(ctx, seg.alloc(home.rec_total));
        RK_HIP(ctx, cur.alloc(2 * home.rec_total));
        RK_HIP(ctx, vals.alloc(most));
        if (home.rec_total) RK_HIP(ctx, hipMemsetAsync(cur.p, 0, (size_t)8 * home.rec_total, stream));
        rk_screen_abund *ab_part = nullptr;
        if (home.rec_total) {
            ab_part = static_cast<rk_screen_abund *>(rk_pool_alloc(ctx, home.rec_total * sizeof(rk_screen_abund)));
            if (!ab_part) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu abundance records on the device", home.rec_total);
            taken_abund.parts.emplace_back(ab_part, home.rec_total);
            RK_HIP(ctx, hipMemsetAsync(ab_part, 0, home.rec_total * sizeof(rk_screen_abund), stream));
            a.seg = seg.p;
            hipLaunchKernelGGL(k_screen_write<true>, dim3(nb), dim3(kScreenThreads), 0, stream, a);
            RK_HIP(ctx, hipGetLastError());
            st->launches++;
        } else {
            RK_HIP(ctx, hipMemsetAsync(won.p, 0, (size_t)nb * N * 4, stream));   // no cell has a record
        }
        for (size_t k = 0; k + 1 < cut.size(); k++) {
            const uint32_t sa = cut[k], sb = cut[k + 1];
            const uint64_t sub_hashes = hoff[s0 + sb] - hoff[s0 + sa], sub_tiles = (sub_hashes + kTileHashes - 1) / kTileHashes;
            const unsigned long long sub_recs = rec_before[sb] - rec_before[sa];
            ab->passes++;
            if (sub_tiles) {
                FillArgs f;
                memset(&f, 0, sizeof f);
                f.q_hashes = qs->wide ? (const void *)qs->d_hashes64 : (const void *)qs->d_hashes;
                f.q_counts = qs->d_counts;
                f.q_off = qs->d_off;
                f.row_of = row_of.p + s0 + sa;
                f.hoff = hoff_dev.p + s0 + sa;
                f.nb = sb - sa;
                f.n_hashes = sub_hashes;
                f.ix = index_lookup_of(idx);
                f.postings = idx->d_postings;
                f.upos = idx->d_upos;
                f.orig = idx->relabeled ? idx->d_orig : nullptr;
                f.sizes_internal = idx->d_sizes;
                f.cnt = counts.p + (size_t)sa * N;
                f.map = won.p + (size_t)sa * N;
                f.n_ref = N;
                f.min_common = o->min_common;
                f.lane_max = st->lane_max;
                f.wave_max = st->wave_max;
                f.seg = seg.p;
                f.cur = cur.p;
                f.vals = vals.p;
                f.vals_cap = std::max<unsigned long long>(1, most);
                f.occ_q = occ_dev.p;
                f.c = abc_dev.p;
                hipLaunchKernelGGL(qs->wide ? k_screen_fill<uint64_t> : k_screen_fill<uint32_t>, dim3((unsigned)sub_tiles), dim3(kScreenThreads), 0, stream, f);
                RK_HIP(ctx, hipGetLastError());
                st->launches++;
            }
            if (sub_recs) {
                SelArgs g;
                memset(&g, 0, sizeof g);
                g.recs = a.recs;
                g.seg = seg.p;
                g.vals = vals.p;
                g.vals_cap = std::max<unsigned long long>(1, most);
                g.out = ab_part;
                g.wave_sel_max = kWaveSelMax;
                g.c = abc_dev.p;
                // a launch takes at most kSelectRecs records: no grid beyond 2^30 workgroups, however many records a sub-range has
                const auto select = [&](unsigned long long first, unsigned long long end, bool by_block) {
                    for (unsigned long long at = first; at < end; at += kSelectRecs) {
                        g.rec_first = at;
                        g.rec_end = std::min(end, at + kSelectRecs);
                        const unsigned long long n = g.rec_end - g.rec_first;
                        if (by_block) hipLaunchKernelGGL(k_screen_select_block, dim3((unsigned)n), dim3(kScreenThreads), 0, stream, g);
                        else hipLaunchKernelGGL(k_screen_select_wave, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kScreenThreads), 0, stream, g);
                        st->launches++;
                    }
                };
                select(rec_before[sa], rec_before[sb], false);
                // the workgroup's select only over the rows that have a record for it (the read-back brought every row's longest segment):
                // one launch per run of such rows, a workgroup per record of the run -- those of its shorter records return at once
                for (uint32_t s = sa; s < sb;) {
                    if (longest_h[s] <= kWaveSelMax) {
                        s++;
                        continue;
                    }
                    uint32_t e = s + 1;
                    while (e < sb && longest_h[e] > kWaveSelMax) e++;
                    select(rec_before[s], rec_before[e], true);
                    s = e;
                }
                RK_HIP(ctx, hipGetLastError());
            }
        }
    }
    // the result in one block, one copy
    const size_t head = Result::head_bytes(Q), bytes = head + total_recs * sizeof(rk_screen_rec);
    DevBuf<unsigned char> block(ctx);
    RK_HIP(ctx, block.alloc(bytes));
    hipLaunchKernelGGL(k_query_scan<kScreenThreads>, dim3(1), dim3(kScreenThreads), 0, stream, per_q.p + 3 * (size_t)Q, (const uint32_t *)nullptr, Q, 0u,
                       (unsigned long long *)block.p, &cnt->all_total);
    RK_HIP(ctx, hipGetLastError());
    st->launches++;
    if (Q) RK_HIP(ctx, hipMemcpyAsync(block.p + ((size_t)Q + 1) * 8, per_q.p + Q, (size_t)4 * Q, hipMemcpyDeviceToDevice, stream));              // matched
    if (Q) RK_HIP(ctx, hipMemcpyAsync(block.p + ((size_t)Q + 1) * 8 + (size_t)4 * Q, per_q.p, (size_t)4 * Q, hipMemcpyDeviceToDevice, stream));   // n_cand
    if (Q) RK_HIP(ctx, hipMemcpyAsync(block.p + ((size_t)Q + 1) * 8 + (size_t)8 * Q, per_q.p + 2 * (size_t)Q, (size_t)4 * Q, hipMemcpyDeviceToDevice, stream));
    size_t at = head;
    for (const auto &p : taken.parts) {
        RK_HIP(ctx, hipMemcpyAsync(block.p + at, p.first, p.second * sizeof(rk_screen_rec), hipMemcpyDeviceToDevice, stream));
        at += p.second * sizeof(rk_screen_rec);
    }
    DevBuf<unsigned char> ab_block(ctx);
    const size_t ab_bytes = total_recs * sizeof(rk_screen_abund) + (size_t)24 * Q + sizeof(AbundCounters);
    if (ab) {   // the abundance records, the sums of the rows and the classes in a block of their own
        RK_HIP(ctx, ab_block.alloc(ab_bytes));
        size_t to = 0;
        for (const auto &p : taken_abund.parts) {
            RK_HIP(ctx, hipMemcpyAsync(ab_block.p + to, p.first, p.second * sizeof(rk_screen_abund), hipMemcpyDeviceToDevice, stream));
            to += p.second * sizeof(rk_screen_abund);
        }
        if (Q) RK_HIP(ctx, hipMemcpyAsync(ab_block.p + to, occ_dev.p, (size_t)24 * Q, hipMemcpyDeviceToDevice, stream));
        RK_HIP(ctx, hipMemcpyAsync(ab_block.p + to + (size_t)24 * Q, abc_dev.p, sizeof(AbundCounters), hipMemcpyDeviceToDevice, stream));
    }
    RK_HIP(ctx, span.end());
    res->block.resize(bytes);
    RK_HIP(ctx, hipMemcpyAsync(res->block.data(), block.p, bytes, hipMemcpyDeviceToHost, stream));
    if (ab) {
        ab->block.resize(ab_bytes);
        RK_HIP(ctx, hipMemcpyAsync(ab->block.data(), ab_block.p, ab_bytes, hipMemcpyDeviceToHost, stream));
    }
    RK_HIP(ctx, hipStreamSynchronize(stream));
    span.read();
    res->n_recs = total_recs;
    if (ab) {
        AbundCounters c;
        memcpy(&c, ab->block.data() + total_recs * sizeof(rk_screen_abund) + (size_t)24 * Q, sizeof c);
        if (c.errors) return rk_fail(ctx, RK_ERR_HIP, "rk_screen_abund_rows: %llu values outside their segments (internal error)", c.errors);
    }
    const uint64_t *off = (const uint64_t *)res->block.data();
    if (off[0] != 0 || off[Q] != total_recs) return rk_fail(ctx, RK_ERR_HIP, "rk_screen_rows: the offsets of the rows do not span the records (internal error)");
    return RK_OK;
}

// what rk_screen_lists and rk_screen_abund_lists refuse alike
int check_lists_args(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off, const uint64_t *q_lists, uint32_t n_query, uint32_t n_ref,
                     const uint32_t *ref_sizes, const uint32_t *query_sizes, const rk_screen_opts *opts, const uint64_t *off_out, rk_screen_rec *const *recs_out,
                     const uint64_t *n_recs, const uint32_t *matched_out, const uint32_t *n_cand_out, const uint32_t *claimed_out)
{
    if (!q_off || !opts || !off_out || !recs_out || !n_recs) return RK_ERR_ARG;
    if (n_query && (!query_sizes || !matched_out || !n_cand_out || !claimed_out)) return RK_ERR_ARG;
    if ((n_lists && !counts) || (n_ref && !ref_sizes) || !opts->min_common) return RK_ERR_ARG;
    if (q_off[0] != 0) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        if (q_off[q + 1] < q_off[q]) return RK_ERR_ARG;
    if (q_off[n_query] && !q_lists) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        for (uint64_t j = q_off[q]; j < q_off[q + 1]; j++)
            if (q_lists[j] >= n_lists || (j > q_off[q] && q_lists[j - 1] >= q_lists[j])) return RK_ERR_ARG;
    for (uint32_t r = 0; r < n_ref; r++)
        if (ref_sizes[r] >= kSizeLimit) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        if (query_sizes[q] >= kSizeLimit) return RK_ERR_ARG;
    uint64_t total = 0;
    for (uint64_t u = 0; u < n_lists; u++) total += counts[u];
    if (total && !postings) return RK_ERR_ARG;
    return RK_OK;
}

// hand_out with the abundance records in memory of their own and the sums of the selected rows; RK_ERR_NOMEM leaves everything untouched
int hand_out_abund(const Result &r, const RowSel &sel, uint32_t Q, uint64_t *off_out, rk_screen_rec **recs_out, rk_screen_abund **abund_out,
                   uint64_t *n_recs, uint32_t *const (&per_row_out)[3], const rk_screen_abund *abund, const uint64_t *occ, uint64_t *occ_out)
{
    rk_screen_abund *p = nullptr;
    if (r.n_recs) {
        p = (rk_screen_abund *)malloc(r.n_recs * sizeof(rk_screen_abund));
        if (!p) return RK_ERR_NOMEM;
        memcpy(p, abund, r.n_recs * sizeof(rk_screen_abund));
    }
    if (hand_out(r, sel, Q, off_out, recs_out, n_recs, per_row_out)) {
        free(p);
        return RK_ERR_NOMEM;
    }
    for (const uint32_t q : sel.rows)
        for (int k = 0; k < 3; k++) occ_out[(size_t)3 * q + k] = occ ? occ[(size_t)3 * q + k] : 0;
    *abund_out = p;
    return RK_OK;
}

// the sums of the counts of the selected sketches at occ[3 q] (the rest 0), from a download: when nothing else runs
int whole_sums(rk_ctx *, const rk_sketches *qs, const RowSel &sel, std::vector<uint64_t> *occ)
{
    std::vector<uint32_t> c(qs->total);
    RK_TRY(rk_sketches_download_counts(qs, c.data()));
    occ->assign((size_t)3 * qs->n, 0);
    for (const uint32_t q : sel.rows)
        for (uint64_t j = qs->h_off[q]; j < qs->h_off[q + 1]; j++) (*occ)[(size_t)3 * q] += c[j];
    return RK_OK;
}

// rk_screen_rows (abund_out == null) and rk_screen_abund_rows.  *full (written on success only) begins with the fields of rk_screen_stats;
// what follows them stays 0 for the plain screen.
int screen_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_screen_opts *opts, uint64_t *off_out, rk_screen_rec **recs_out,
                rk_screen_abund **abund_out, uint64_t *n_recs, uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *claimed_out, uint64_t *occ_out,
                rk_screen_abund_stats *full)
{
    static_assert(offsetof(rk_screen_abund_stats, values) == sizeof(rk_screen_stats), "rk_screen_abund_stats begins with rk_screen_stats");
    rk_screen_abund_stats more;   // what rk_screen_abund_stats adds
    memset(&more, 0, sizeof more);
    rk_screen_abund_stats *const ast = &more;
    if (!ctx || !idx || !queries || !opts || !off_out || !recs_out || !n_recs) return RK_ERR_ARG;
    const bool abund = abund_out != nullptr;
    const char *const who = abund ? "rk_screen_abund_rows" : "rk_screen_rows";
    const uint32_t N = idx->n_ref, Q = queries->n;
    if (abund && Q && !occ_out) return rk_fail(ctx, RK_ERR_ARG, "%s: occ_out is null", who);
    if (abund && !queries->d_counts) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: the query sketches carry no counts (rk_sketches_has_counts)", who);
    if (Q && (!matched_out || !n_cand_out || !claimed_out)) return rk_fail(ctx, RK_ERR_ARG, "%s: matched_out, n_cand_out or claimed_out is null", who);
    if (!opts->min_common) return rk_fail(ctx, RK_ERR_ARG, "%s: min_common must be at least 1", who);
    if (queries->wide != idx->wide) return rk_fail(ctx, RK_ERR_ARG, "query sketches and index use different hash widths");
    if (N && (!idx->d_postings || !idx->d_upos || idx->n_shards > 1))
        return rk_fail(ctx, RK_ERR_ARG, "%s: an index without all posting lists (rk_index_join_shard, one hash range of a sharded build)", who);
    if (N && Q && (!idx->ref_sets || !queries->is_set)) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s takes sketches as sets: a sketch repeats a hash", who);
    if (idx->H >= 0x7FFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "explicit queries against an index of 2^31-1 postings or more");
    if (N && Q && (idx->max_ref_size >= kSizeLimit || queries->max_size >= kSizeLimit))
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: a sketch of 2^30 hashes or more (the products of the comparison stay below 2^60)", who);
    rk_screen_stats st;
    memset(&st, 0, sizeof st);
    fill_constants(&st);
    const TimedSpan span{ctx, abund ? RK_MS_SCREEN_ABUND : RK_MS_SCREEN};
    span.clear();
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, Q);
    AbundDevice ab;
    st.rows = (uint32_t)sel.rows.size();
    uint32_t *const outs[3] = {matched_out, n_cand_out, claimed_out};
    HostResult host;
    DeviceResult dev;
    Result r;
    const bool runs = N && !sel.rows.empty();   // (else every row is empty: r stays without offsets)
    if (runs && rk_switched_off("RK_SCREEN_DEVICE")) {
        st.path = 2;
        RK_TRY(idx->wide ? screen_on_host<uint64_t>(ctx, idx, queries, opts, sel, abund, &host) : screen_on_host<uint32_t>(ctx, idx, queries, opts, sel, abund, &host));
        r = view(host);
        st.postings_walked = host.walked;
        st.lane_lists = host.lane_lists;
        st.wave_lists = host.wave_lists;
        st.block_lists = host.block_lists;
        st.batches = 1;
        st.rows_per_batch = sel.rows.size();
    } else if (runs) {
        st.path = 1;
        RK_TRY(screen_on_device(ctx, idx, queries, opts, sel, &st, &dev, abund ? &ab : nullptr));
        r = Result::from_block(dev.block.data(), Q, dev.n_recs);
    }
    if (abund) {
        const rk_screen_abund *recs_ab = nullptr;
        const uint64_t *occ = nullptr;
        ast->rank_max = kRankMax;
        ast->wave_sel_max = kWaveSelMax;
        ast->chunk = kScreenThreads;
        if (st.path == 2) {
            recs_ab = host.abund.data();
            occ = host.occ.data();
            ast->values = host.values;
            ast->rank_segs = host.rank_segs;
            ast->wave_segs = host.wave_segs;
            ast->block_segs = host.block_segs;
        } else if (st.path == 1) {
            recs_ab = (const rk_screen_abund *)ab.block.data();
            occ = (const uint64_t *)(ab.block.data() + dev.n_recs * sizeof(rk_screen_abund));
            AbundCounters c;
            memcpy(&c, ab.block.data() + dev.n_recs * sizeof(rk_screen_abund) + (size_t)24 * Q, sizeof c);
            ast->values = ab.values;
            ast->value_bytes = ab.value_bytes;
            ast->value_passes = ab.passes;
            ast->rank_segs = c.rank_segs;
            ast->wave_segs = c.wave_segs;
            ast->block_segs = c.block_segs;
        }
        if (st.path == 0 && Q && !N) {   // an index without genomes: the sums of the whole sketches are still the queries'
            RK_TRY(whole_sums(ctx, queries, sel, &host.occ));
            occ = host.occ.data();
        }
        if (hand_out_abund(r, sel, Q, off_out, recs_out, abund_out, n_recs, outs, recs_ab, occ, occ_out)) return rk_fail(ctx, RK_ERR_NOMEM, "%s: out of host memory", who);
    } else if (hand_out(r, sel, Q, off_out, recs_out, n_recs, outs)) {
        return rk_fail(ctx, RK_ERR_NOMEM, "%s: out of host memory", who);
    }
    st.records = r.n_recs;
    for (const uint32_t q : sel.rows) {
        st.matched += matched_out[q];
        st.candidates += n_cand_out[q];
        st.claimed += claimed_out[q];
    }
    memcpy(&more, &st, sizeof st);
    *full = more;
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_screen_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off, const uint64_t *q_lists, uint32_t n_query,
                    uint32_t n_ref, const uint32_t *ref_sizes, const uint32_t *query_sizes, const rk_screen_opts *opts, uint64_t *off_out,
                    rk_screen_rec **recs_out, uint64_t *n_recs, uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *claimed_out)
{
    if (int rc = check_lists_args(postings, counts, n_lists, q_off, q_lists, n_query, n_ref, ref_sizes, query_sizes, opts, off_out, recs_out, n_recs, matched_out,
                                  n_cand_out, claimed_out))
        return rc;
    std::vector<uint64_t> pos;
    std::vector<uint32_t> fixed;
    const uint32_t *post = nullptr;
    if (int rc = prepare_lists(postings, counts, n_lists, n_ref, &pos, &fixed, &post)) return rc;
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, n_query);
    HostResult r;
    if (int rc = screen_core(post, pos.data(), q_off, q_lists, nullptr, n_query, n_ref, ref_sizes, query_sizes, opts, sel, true, &r)) return rc;
    return hand_out(view(r), sel, n_query, off_out, recs_out, n_recs, {matched_out, n_cand_out, claimed_out});
}

int rk_screen_abund_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off, const uint64_t *q_lists, const uint32_t *q_counts,
                          uint32_t n_query, uint32_t n_ref, const uint32_t *ref_sizes, const uint32_t *query_sizes, const uint64_t *query_occ, const rk_screen_opts *opts,
                          uint64_t *off_out, rk_screen_rec **recs_out, rk_screen_abund **abund_out, uint64_t *n_recs, uint32_t *matched_out, uint32_t *n_cand_out,
                          uint32_t *claimed_out, uint64_t *occ_out)
{
    if (int rc = check_lists_args(postings, counts, n_lists, q_off, q_lists, n_query, n_ref, ref_sizes, query_sizes, opts, off_out, recs_out, n_recs, matched_out,
                                  n_cand_out, claimed_out))
        return rc;
    if (!abund_out || (n_query && (!occ_out || !query_occ)) || (q_off[n_query] && !q_counts)) return RK_ERR_ARG;
    for (uint64_t j = 0; j < q_off[n_query]; j++)
        if (!q_counts[j]) return RK_ERR_ARG;
    std::vector<uint64_t> pos;
    std::vector<uint32_t> fixed;
    const uint32_t *post = nullptr;
    if (int rc = prepare_lists(postings, counts, n_lists, n_ref, &pos, &fixed, &post)) return rc;
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, n_query);
    HostResult r;
    static const uint32_t none = 0;   // (no query hits a list: q_counts may be null)
    if (int rc = screen_core(post, pos.data(), q_off, q_lists, q_counts ? q_counts : &none, n_query, n_ref, ref_sizes, query_sizes, opts, sel, true, &r)) return rc;
    for (const uint32_t q : sel.rows) r.occ[(size_t)3 * q] = query_occ[q];
    return hand_out_abund(view(r), sel, n_query, off_out, recs_out, abund_out, n_recs, {matched_out, n_cand_out, claimed_out}, r.abund.data(), r.occ.data(), occ_out);
}

int rk_screen_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_screen_opts *opts, uint64_t *off_out, rk_screen_rec **recs_out,
                   uint64_t *n_recs, uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *claimed_out, rk_screen_stats *stats)
{
    rk_screen_abund_stats full;
    RK_TRY(screen_rows(ctx, idx, queries, opts, off_out, recs_out, nullptr, n_recs, matched_out, n_cand_out, claimed_out, nullptr, &full));
    if (stats) memcpy(stats, &full, sizeof *stats);
    return RK_OK;
}

int rk_screen_abund_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_screen_opts *opts, uint64_t *off_out, rk_screen_rec **recs_out,
                         rk_screen_abund **abund_out, uint64_t *n_recs, uint32_t *matched_out, uint32_t *n_cand_out, uint32_t *claimed_out, uint64_t *occ_out,
                         rk_screen_abund_stats *stats)
{
    if (!abund_out) return RK_ERR_ARG;
    rk_screen_abund_stats full;
    RK_TRY(screen_rows(ctx, idx, queries, opts, off_out, recs_out, abund_out, n_recs, matched_out, n_cand_out, claimed_out, occ_out, &full));
    if (stats) *stats = full;
    return RK_OK;
}

}  // extern "C"
