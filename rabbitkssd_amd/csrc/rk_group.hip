// rk_group.hip -- pan, core and marker sketches per cluster (rk_group_sketches) from the posting lists of an index, and the same rule on
// the host over exported lists (rk_group_lists).  labels[v] < N names v's cluster, RK_GROUP_NONE leaves v unlabelled; the groups are the
// labels in use by ascending label.  For a hash h: c_g(h) = the distinct genomes of group g that hold h, t(h) = the distinct genomes that
// hold h.  h is in the sketch of g iff c >= need[g] = max(min_count, ceil(share_num * m_g / share_den)) and, with `only`, c == t.  Whether
// h belongs to g depends on h's posting list alone: no join, no distance.  include/rabbitkssd.h, pan, core and marker sketches.
//
//   host      the group number of every genome and need[] (host arithmetic), uploaded once: 4 N + 4 K bytes;
//   gather    k_group_numbers: the group numbers in INTERNAL genome order through d_orig (an imported index: the upload itself);
//   lists     by the length of a list, since lengths span 1 to N:
//             k_group_lane   up to kLaneMax postings: one lane per list, the group numbers in registers, compared pairwise; lanes of a
//                            wave take neighbouring lists, so their posting reads touch one contiguous span.  The same sweep queues the
//                            longer lists for the two kernels below (one wave-aggregated reservation per queue);
//             k_group_wave   up to kWaveMax postings: one wave per list, one posting per lane, the groups peeled off by ballots (one
//                            round per distinct group) -- no LDS; kWaveBatch lists per trip, so that their loads are in flight together;
//             k_group_block  longer lists: one workgroup per list streams it in chunks of kChunk postings into an LDS table keyed by
//                            group number (LDS atomics).  Internal order puts relatives next to each other: a long list has few
//                            groups.  A list with more than kTableGroups groups is SPILLED: its raw keys list << 32 | group, and
//                            list << 32 | ~0 per distinct genome, go to a global buffer;
//             every (list u, group g) that passes appends the key g << 32 | u to the record buffer: ONE atomic reservation per wave
//             (wave_reserve here, wave_append of rk_query_dev.h), not one per lane;
//   spill     rk_prim_sort_keys_u64 + rk_prim_rle_u64 over the raw keys: a run IS c_g(h), the run of ~0 is t(h); k_group_spill_emit
//             applies the rule (t by binary search among the runs) and appends to the same record buffer;
//   overflow  the counters keep counting past the capacities; the call then runs once more with the exact counts (attempts = 2);
//   sort      the keys over the bits in use (32 + bits of K).  u ascends with the hash: the sorted keys ARE the result's order;
//   offsets   k_group_offsets: a lower bound per group, K + 1 offsets;
//   hashes    k_group_hashes: d_uhash[u] / d_uhash64[u] into the new object's hash array.
//
// Memory scope: every array is written by one kernel and read by a later one on the same stream.  INSIDE a launch the only communication
// is relaxed agent-scope atomic adds on the counters (reservations: nobody reads what another thread wrote) and, in k_group_block, LDS
// atomics between barriers.  No loop waits for another workgroup: any grid works.  The host synchronises once for the counters before the
// sort (once more behind a spill) and once for the offsets.  DESIGN.md 4.14.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "rk_internal.h"
#include "rk_query_dev.h"

namespace {

constexpr uint32_t kNone = RK_GROUP_NONE;
constexpr uint32_t kDup = 0xFFFFFFFEu;     // a posting that repeats the genome before it (group numbers lie below 2^31)
constexpr int kLaneMax = 8;                // k_group_lane: the longest list one lane takes
constexpr int kWaveMax = 64;               // k_group_wave: the longest list one wave takes (one posting per lane)
constexpr int kChunk = 256;                // k_group_block: threads of the workgroup = postings of one chunk
constexpr int kTableBits = 9, kTableSlots = 1 << kTableBits;
constexpr int kTableGroups = 256;          // distinct groups of one list the LDS table holds (half its slots: short probe chains)
static_assert(kWaveMax == 64 && kChunk % 64 == 0 && kTableGroups + kChunk <= kTableSlots, "one chunk past a full table still finds a free slot");
static_assert(sizeof(rk_group_rule) == 16 && sizeof(rk_group_stats) == 88, "the layouts of include/rabbitkssd.h");

struct Counters {   // one device block, read back in one copy
    unsigned long long n_rec, n_spill, n_wave, n_block, spilled, n_runs;
};

struct ListArgs {
    const uint32_t *postings, *upos;   // the index: u32[H], u32[U + 1]
    const uint32_t *grp, *need;        // group number per INTERNAL genome id (kNone: unlabelled), need per group
    unsigned long long U;
    uint32_t only;
    unsigned long long *rec, rec_cap;      // g << 32 | u
    unsigned long long *spill, spill_cap;  // u << 32 | g, u << 32 | ~0
    uint32_t *wave_q, *block_q;            // the lists of the two longer classes
    Counters *cnt;
};

// Every lane of a full wave calls it in converged code.  wave_reserve: room for n_mine entries per lane behind *counter, one atomic
// per wave; returns where this lane's entries begin (the counter counts past any capacity: the caller checks each slot).
__device__ __forceinline__ unsigned long long wave_reserve(uint32_t n_mine, unsigned long long *counter)
{
    const int lane = threadIdx.x & 63;
    uint32_t incl = n_mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += v;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    if (!total) return 0;   // (uniform)
    unsigned long long base = 0;
    if (lane == 63) base = add_u64(counter, total);
    return shfl_u64(base, 63) + incl - n_mine;
}

__device__ __forceinline__ bool passes(uint32_t c, uint32_t t, uint32_t need, uint32_t only) { return c >= need && (!only || c == t); }

// the caller's group numbers in the index's internal genome order
__global__ void k_group_numbers(const uint32_t *grp_caller, const uint32_t *orig, uint32_t n, uint32_t *grp)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) grp[i] = grp_caller[orig[i]];   // (orig[] < n: rk_index_build's permutation, checked on every import of a blob)
}

// One lane per list; the lists of up to kLaneMax postings are decided here, the longer ones queued.  wave_q has room for every list of
// more than kLaneMax postings, block_q for every list of more than kWaveMax (the host sized them from H).  The loads of a lane do not
// depend on each other's values: all postings first (a slot beyond the list reads posting 0 and is masked afterwards), then all group
// numbers -- two round trips to memory per list, not sixteen.
__global__ void __launch_bounds__(kChunk) k_group_lane(ListArgs a)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long wave = ((unsigned long long)blockIdx.x * kChunk + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * (kChunk / 64);
    for (unsigned long long first = wave * 64; first < a.U; first += n_waves * 64) {   // (uniform per wave)
        const unsigned long long u = first + lane;
        uint32_t beg = 0, len = 0;
        if (u < a.U) {
            beg = a.upos[u];
            len = a.upos[u + 1] - beg;
        }
        const bool to_wave = len > (uint32_t)kLaneMax && len <= (uint32_t)kWaveMax, to_block = len > (uint32_t)kWaveMax;
        const uint32_t wq = queue_slot(to_wave, &a.cnt->n_wave), bq = queue_slot(to_block, &a.cnt->n_block);
        if (to_wave) a.wave_q[wq] = (uint32_t)u;
        if (to_block) a.block_q[bq] = (uint32_t)u;
        const uint32_t mine_len = len <= (uint32_t)kLaneMax ? len : 0u;
        uint32_t p[kLaneMax], g[kLaneMax], t = 0;
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) p[j] = a.postings[(uint32_t)j < mine_len ? beg + j : 0u];   // (U > 0: posting 0 exists)
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) g[j] = a.grp[p[j]];
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) {
            const bool fresh = (uint32_t)j < mine_len && (j == 0 || p[j] != p[j > 0 ? j - 1 : 0]);
            if (!fresh) g[j] = kDup;
            t += fresh;
        }
        uint32_t c[kLaneMax], first_mask = 0;
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) {
            c[j] = 0;
            bool first_of_group = g[j] < kDup;   // not a repeat, an unlabelled genome or beyond the list
#pragma unroll
            for (int i = 0; i < kLaneMax; i++) {
                c[j] += g[i] == g[j];
                if (i < j && g[i] == g[j]) first_of_group = false;
            }
            if (first_of_group) first_mask |= 1u << j;
        }
        uint32_t pass = 0;
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) {
            const uint32_t need = a.need[first_mask >> j & 1u ? g[j] : 0u];   // (a group 0 exists)
            if ((first_mask >> j & 1u) && passes(c[j], t, need, a.only)) pass |= 1u << j;
        }
        unsigned long long at = wave_reserve((uint32_t)__popc(pass), &a.cnt->n_rec);
#pragma unroll
        for (int j = 0; j < kLaneMax; j++)
            if (pass >> j & 1u) {
                if (at < a.rec_cap) a.rec[at] = ((unsigned long long)g[j] << 32) | u;
                at++;
            }
    }
}

// One wave per queued list of kLaneMax < len <= kWaveMax postings, one posting per lane.  A wave takes 64 queue entries at a time (their
// list numbers and bounds: one load per lane) and works through them kWaveBatch lists at a time: the postings of the batch, then their
// group numbers, then the ballots, then the batch's need[] -- the loads of a batch are in flight together, and the batch makes ONE
// reservation.  (One list per trip waited for five dependent loads and an atomic each time: 2.4 ms for 614,000 lists.)
constexpr int kWaveBatch = 8;
__global__ void __launch_bounds__(kChunk) k_group_wave(ListArgs a)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long wave = ((unsigned long long)blockIdx.x * kChunk + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * (kChunk / 64);
    const unsigned long long n = a.cnt->n_wave;   // (final: k_group_lane is through)
    for (unsigned long long first = wave * 64; first < n; first += n_waves * 64) {   // (uniform per wave)
        uint32_t u_l = 0, beg_l = 0, len_l = 0;   // lane l: queue entry first + l (len 0 beyond the queue)
        if (first + lane < n) {
            u_l = a.wave_q[first + lane];
            beg_l = a.upos[u_l];
            len_l = a.upos[u_l + 1] - beg_l;
        }
        const int here = (int)(n - first < 64 ? n - first : 64);
        for (int k0 = 0; k0 < here; k0 += kWaveBatch) {   // (uniform; k0 + kWaveBatch <= 64)
            uint32_t p[kWaveBatch], g[kWaveBatch], c[kWaveBatch], t[kWaveBatch];
            bool valid[kWaveBatch];
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) {
                const uint32_t beg = (uint32_t)__shfl((int)beg_l, k0 + j), len = (uint32_t)__shfl((int)len_l, k0 + j);
                valid[j] = (uint32_t)lane < len;
                p[j] = a.postings[valid[j] ? beg + lane : 0u];
            }
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) g[j] = a.grp[p[j]];
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) {
                const uint32_t before = (uint32_t)__shfl_up((int)p[j], 1);
                const bool fresh = valid[j] && (lane == 0 || p[j] != before);
                if (!fresh) g[j] = kDup;
                t[j] = (uint32_t)__popcll(__ballot(fresh));
                c[j] = 0;
                unsigned long long pending = __ballot(g[j] < kDup);
                while (pending) {   // (uniform) one round per distinct group; its first lane keeps the count
                    const int lead = __ffsll((long long)pending) - 1;
                    const uint32_t gl = (uint32_t)__shfl((int)g[j], lead);
                    const unsigned long long m = __ballot(g[j] == gl);
                    if (lane == lead) c[j] = (uint32_t)__popcll(m);
                    pending &= ~m;
                }
            }
            uint32_t pass = 0;
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) {
                const uint32_t need = a.need[c[j] ? g[j] : 0u];   // (a group 0 exists)
                if (c[j] && passes(c[j], t[j], need, a.only)) pass |= 1u << j;
            }
            unsigned long long at = wave_reserve((uint32_t)__popc(pass), &a.cnt->n_rec);
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) {
                const uint32_t u = (uint32_t)__shfl((int)u_l, k0 + j);
                if (pass >> j & 1u) {
                    if (at < a.rec_cap) a.rec[at] = ((unsigned long long)g[j] << 32) | u;
                    at++;
                }
            }
        }
    }
}

// One workgroup per queued list of more than kWaveMax postings
__global__ void __launch_bounds__(kChunk) k_group_block(ListArgs a)
{
    __shared__ uint32_t s_key[kTableSlots], s_cnt[kTableSlots];
    __shared__ uint32_t s_t, s_groups, s_over;
    const uint32_t tid = threadIdx.x;
    const unsigned long long n = a.cnt->n_block;   // (final: k_group_lane is through)
    for (unsigned long long i = blockIdx.x; i < n; i += gridDim.x) {   // (uniform per workgroup)
        const uint32_t u = a.block_q[i];
        const uint32_t beg = a.upos[u], len = a.upos[u + 1] - beg;
        for (uint32_t s = tid; s < (uint32_t)kTableSlots; s += kChunk) {
            s_key[s] = kNone;
            s_cnt[s] = 0;
        }
        if (tid == 0) s_t = s_groups = s_over = 0;
        __syncthreads();
        uint32_t t_mine = 0;
        bool over = false;
        for (uint32_t base = 0; base < len && !over; base += kChunk) {   // (uniform: `over` is read behind a barrier)
            const uint32_t k = base + tid;
            if (k < len) {
                const uint32_t p = a.postings[beg + k];
                const uint32_t g = (k == 0 || a.postings[beg + k - 1] != p) ? a.grp[p] : kDup;
                if (g != kDup) t_mine++;
                if (g < kDup) {
                    // at most kTableGroups groups sit in the table when a chunk begins and a chunk adds at most kChunk: a free slot exists
                    uint32_t slot = (g * 0x9E3779B1u) >> (32 - kTableBits);
                    bool done = false;
                    for (int probe = 0; probe < kTableSlots && !done; probe++) {
                        const uint32_t old = atomicCAS(&s_key[slot], kNone, g);
                        if (old == kNone && atomicAdd(&s_groups, 1u) >= (uint32_t)kTableGroups) atomicExch(&s_over, 1u);
                        if (old == kNone || old == g) {
                            atomicAdd(&s_cnt[slot], 1u);
                            done = true;
                        }
                        slot = (slot + 1) & (kTableSlots - 1);
                    }
                    if (!done) atomicExch(&s_over, 1u);
                }
            }
            __syncthreads();
            over = s_over != 0;
            __syncthreads();   // (nobody sets s_over in the next chunk before everybody has read it)
        }
        if (over) {
            // more groups than the table holds: the raw keys of the whole list, counted by sort + run lengths (k_group_spill_emit)
            if (tid == 0) add_u64(&a.cnt->spilled, 1ULL);
            for (uint32_t base = 0; base < len; base += kChunk) {   // (uniform)
                const uint32_t k = base + tid;
                uint32_t g = kDup;
                if (k < len) {
                    const uint32_t p = a.postings[beg + k];
                    if (k == 0 || a.postings[beg + k - 1] != p) g = a.grp[p];
                }
                unsigned long long at = wave_reserve(g == kDup ? 0u : (g == kNone ? 1u : 2u), &a.cnt->n_spill);
                if (g < kDup) {
                    if (at < a.spill_cap) a.spill[at] = ((unsigned long long)u << 32) | g;
                    at++;
                }
                if (g != kDup && at < a.spill_cap) a.spill[at] = ((unsigned long long)u << 32) | kNone;
            }
        } else {
            if (t_mine) atomicAdd(&s_t, t_mine);
            __syncthreads();
            const uint32_t t = s_t;
            for (uint32_t s = tid; s < (uint32_t)kTableSlots; s += kChunk) {   // (uniform: kTableSlots is a multiple of kChunk)
                const uint32_t g = s_key[s];
                const bool mine = g != kNone && passes(s_cnt[s], t, a.need[g], a.only);
                wave_append(mine, ((unsigned long long)g << 32) | u, &a.cnt->n_rec, a.rec, a.rec_cap);
            }
        }
        __syncthreads();   // the table is reset for the next list
    }
}

// The spilled lists: runs[] = the distinct raw keys ascending, counts[] their multiplicities, *n_runs of them.  A run (u, g) is c_g of
// list u, the run (u, ~0) -- the last of its list -- is t.
__global__ void __launch_bounds__(kChunk) k_group_spill_emit(const unsigned long long *runs, const unsigned int *counts, const unsigned long long *n_runs_dev,
                                                            const uint32_t *need, uint32_t only, unsigned long long *rec, unsigned long long rec_cap,
                                                            unsigned long long *n_rec)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long wave = ((unsigned long long)blockIdx.x * kChunk + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * (kChunk / 64);
    const unsigned long long n = *n_runs_dev;
    for (unsigned long long first = wave * 64; first < n; first += n_waves * 64) {   // (uniform per wave)
        const unsigned long long i = first + lane;
        bool mine = false;
        unsigned long long key = 0;
        if (i < n) {
            const unsigned long long r = runs[i];
            const uint32_t g = (uint32_t)r;
            if (g != kNone) {
                uint32_t t = 0;
                if (only) {   // the run (u, ~0): the first run at or above it
                    const unsigned long long want = r | 0xFFFFFFFFULL;
                    unsigned long long lo = i, hi = n;   // runs[lo] < want <= runs[hi] (hi = n: none)
                    while (hi - lo > 1) {
                        const unsigned long long mid = (lo + hi) >> 1;
                        if (runs[mid] < want) lo = mid; else hi = mid;
                    }
                    t = hi < n && runs[hi] == want ? counts[hi] : 0u;   // (absent: nothing passes)
                }
                mine = passes(counts[i], t, need[g], only);
                key = ((unsigned long long)g << 32) | (r >> 32);
            }
        }
        wave_append(mine, key, n_rec, rec, rec_cap);
    }
}

// off[g] = the first sorted key of group g or a later one, g = 0 .. K (off[K] = n)
__global__ void k_group_offsets(const unsigned long long *sorted, unsigned long long n, uint32_t K, uint64_t *off)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > K) return;
    const unsigned long long want = (unsigned long long)g << 32;
    unsigned long long lo = 0, hi = n;   // keys below lo are < want, keys from hi on are >= want
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (sorted[mid] < want) lo = mid + 1; else hi = mid;
    }
    off[g] = lo;
}

template <class Hash> __global__ void k_group_hashes(const unsigned long long *sorted, unsigned long long n, const Hash *uhash, Hash *out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = uhash[(uint32_t)sorted[i]];   // (a key's low half is a list number below U: the list kernels wrote it)
}

// ---- host: the rule, exactly ------------------------------------------------------------------------------------------------
bool rule_ok(const rk_group_rule *r) { return r->share_den >= 1 && r->share_num <= r->share_den && r->min_count >= 1 && r->only <= 1; }

// the groups of a labelling: the group number of every genome (kNone: unlabelled), the label, size and need of every group
struct Groups {
    std::vector<uint32_t> number, label, size, need;
    uint32_t labelled = 0;
    uint32_t count() const { return (uint32_t)label.size(); }
};

// RK_ERR_ARG for a label that is neither below n nor RK_GROUP_NONE
int make_groups(const uint32_t *labels, uint32_t n, const rk_group_rule *rule, Groups *out)
{
    for (uint32_t v = 0; v < n; v++)
        if (labels[v] >= n && labels[v] != kNone) return RK_ERR_ARG;
    std::vector<uint32_t> members(n, 0), at(n, kNone);
    for (uint32_t v = 0; v < n; v++)
        if (labels[v] != kNone) {
            members[labels[v]]++;
            out->labelled++;
        }
    for (uint32_t l = 0; l < n; l++)
        if (members[l]) {
            at[l] = out->count();
            out->label.push_back(l);
            out->size.push_back(members[l]);
            const uint64_t share = ((uint64_t)rule->share_num * members[l] + rule->share_den - 1) / rule->share_den;   // c * den >= num * m  <=>  c >= ceil(num * m / den)
            out->need.push_back((uint32_t)std::max<uint64_t>(rule->min_count, share));
        }
    out->number.resize(n);
    for (uint32_t v = 0; v < n; v++) out->number[v] = labels[v] == kNone ? kNone : at[labels[v]];
    return RK_OK;
}

template <class T> T *host_copy(const std::vector<T> &v)
{
    T *p = (T *)malloc((v.size() ? v.size() : 1) * sizeof(T));
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

void fill_constants(rk_group_stats *st)
{
    st->lane_max = kLaneMax;
    st->wave_max = kWaveMax;
    st->table_groups = kTableGroups;
    st->chunk = kChunk;
}

// the rule over lists in the caller's genome ids: per group the indices of the kept lists, ascending (off: K + 1, kept: off[K])
void group_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const Groups &gr, uint32_t only, std::vector<uint64_t> *off,
                 std::vector<uint64_t> *kept)
{
    const uint32_t K = gr.count();
    std::vector<std::pair<uint32_t, uint64_t>> pairs;   // (group, list), lists ascending
    std::vector<uint32_t> c(K, 0), touched, list;
    uint64_t at = 0;
    for (uint64_t u = 0; u < n_lists; u++) {
        list.assign(postings + at, postings + at + counts[u]);
        at += counts[u];
        std::sort(list.begin(), list.end());
        list.erase(std::unique(list.begin(), list.end()), list.end());
        const uint32_t t = (uint32_t)list.size();
        touched.clear();
        for (uint32_t v : list) {
            const uint32_t g = gr.number[v];
            if (g != kNone && !c[g]++) touched.push_back(g);
        }
        for (uint32_t g : touched) {
            if (c[g] >= gr.need[g] && (!only || c[g] == t)) pairs.emplace_back(g, u);
            c[g] = 0;
        }
    }
    off->assign((size_t)K + 1, 0);
    for (const auto &p : pairs) (*off)[p.first + 1]++;
    for (uint32_t g = 0; g < K; g++) (*off)[g + 1] += (*off)[g];
    kept->resize(pairs.size());
    std::vector<uint64_t> next(off->begin(), off->end() - 1);
    for (const auto &p : pairs) (*kept)[next[p.first]++] = p.second;
}

unsigned long long env_cap(const char *name, unsigned long long otherwise)
{
    const char *sw = getenv(name);
    const unsigned long long v = sw ? strtoull(sw, nullptr, 10) : 0;
    return v ? v : otherwise;
}

unsigned grid_for(rk_ctx *ctx, unsigned long long items, unsigned long long per_block)
{
    const unsigned long long want = (items + per_block - 1) / per_block, most = (unsigned long long)std::max(1, ctx->num_cu) * 8;
    return (unsigned)std::max<unsigned long long>(1, std::min(want, most));
}

// RK_GROUP_DEVICE=0: export + rk_group_lists + gather + rk_sketches_from_host(64)
template <class Hash> int group_on_host(rk_ctx *ctx, const rk_index *idx, const Groups &gr, uint32_t only, rk_sketches **out)
{
    std::vector<uint32_t> postings(idx->H), counts(idx->U);
    std::vector<Hash> hashes(idx->U);
    if constexpr (sizeof(Hash) == 8) RK_TRY(rk_index_export64(idx, postings.data(), hashes.data(), counts.data()));
    else RK_TRY(rk_index_export_lists(idx, postings.data(), hashes.data(), counts.data()));
    std::vector<uint64_t> off, kept;
    group_lists(postings.data(), counts.data(), idx->U, gr, only, &off, &kept);
    std::vector<Hash> h(kept.size());
    for (size_t i = 0; i < kept.size(); i++) h[i] = hashes[kept[i]];
    if constexpr (sizeof(Hash) == 8) return rk_sketches_from_host64(ctx, h.data(), off.data(), gr.count(), out);
    else return rk_sketches_from_host(ctx, h.data(), off.data(), gr.count(), out);
}

int group_on_device(rk_ctx *ctx, const rk_index *idx, const Groups &gr, uint32_t only, rk_group_stats *st, rk_sketches **out)
{
    const uint32_t N = idx->n_ref, K = gr.count();
    const unsigned long long U = idx->U, H = idx->H;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const TimedSpan span{ctx, RK_MS_GROUP};
    DevBuf<uint32_t> grp_caller(ctx), grp(ctx), need(ctx), wave_q(ctx), block_q(ctx);
    DevBuf<Counters> cnt(ctx);
    RK_HIP(ctx, grp_caller.alloc(N));
    RK_HIP(ctx, need.alloc(K));
    RK_HIP(ctx, cnt.alloc(1));
    // every list of more than kLaneMax (kWaveMax) postings has a slot
    RK_HIP(ctx, wave_q.alloc(std::min(U, H / (kLaneMax + 1)) + 1));
    RK_HIP(ctx, block_q.alloc(std::min(U, H / (kWaveMax + 1)) + 1));
    // (pageable memory of this function: the read-back of the counters synchronises the stream before it returns)
    RK_HIP(ctx, hipMemcpyAsync(grp_caller.p, gr.number.data(), (size_t)N * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemcpyAsync(need.p, gr.need.data(), (size_t)K * 4, hipMemcpyHostToDevice, stream));
    const uint32_t *grp_internal = grp_caller.p;
    if (idx->relabeled && idx->d_orig) {
        RK_HIP(ctx, grp.alloc(N));
        hipLaunchKernelGGL(k_group_numbers, dim3(blocks_for(N)), dim3(kThreads), 0, stream, grp_caller.p, idx->d_orig, N, grp.p);
        RK_HIP(ctx, hipGetLastError());
        grp_internal = grp.p;
    }
    // a record needs a posting of its own: H bounds both buffers
    unsigned long long rec_cap = std::min(std::max(H, 1ULL), env_cap("RK_GROUP_CAP", U + U / 2 + 4096));
    unsigned long long spill_cap = std::min(std::max(2 * H, 1ULL), env_cap("RK_GROUP_SPILL_CAP", H / 4 + (1ULL << 17)));
    DevBuf<unsigned long long> rec(ctx), spill(ctx), spill_sorted(ctx), runs(ctx), sorted(ctx);
    DevBuf<unsigned int> run_counts(ctx);
    Counters home;
    memset(&home, 0, sizeof home);
    for (st->attempts = 1;; st->attempts++) {
        RK_HIP(ctx, rec.alloc(rec_cap));
        RK_HIP(ctx, spill.alloc(spill_cap));
        RK_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(Counters), stream));
        RK_HIP(ctx, span.begin());
        if (U) {
            const ListArgs a{idx->d_postings, idx->d_upos, grp_internal, need.p, U, only, rec.p, rec_cap, spill.p, spill_cap, wave_q.p, block_q.p, cnt.p};
            hipLaunchKernelGGL(k_group_lane, dim3(grid_for(ctx, U, kChunk)), dim3(kChunk), 0, stream, a);
            hipLaunchKernelGGL(k_group_wave, dim3(grid_for(ctx, std::min(U, H / (kLaneMax + 1)) + 1, kChunk / 64)), dim3(kChunk), 0, stream, a);
            hipLaunchKernelGGL(k_group_block, dim3(grid_for(ctx, std::min(U, H / (kWaveMax + 1)) + 1, 1)), dim3(kChunk), 0, stream, a);
            RK_HIP(ctx, hipGetLastError());
        }
        RK_TRY(rk_read_back(ctx, &home, cnt.p, sizeof home, stream));   // the one synchronisation before the sort
        if (home.n_wave > std::min(U, H / (kLaneMax + 1)) || home.n_block > std::min(U, H / (kWaveMax + 1)))
            return rk_fail(ctx, RK_ERR_HIP, "rk_group_sketches: more long lists than the postings allow (internal error)");
        bool again = home.n_rec > rec_cap || home.n_spill > spill_cap;
        if (again) {   // a labelled raw key of a spilled list gives at most one record
            rec_cap = std::max(rec_cap, home.n_rec + home.n_spill / 2);
            spill_cap = std::max(spill_cap, home.n_spill);
        } else if (home.n_spill) {
            const unsigned long long ns = home.n_spill;
            RK_HIP(ctx, spill_sorted.alloc(ns));
            RK_HIP(ctx, runs.alloc(ns));
            RK_HIP(ctx, run_counts.alloc(ns));
            RK_TRY(rk_prim_sort_keys_u64(ctx, spill.p, spill_sorted.p, ns, 0, 64, stream));
            RK_TRY(rk_prim_rle_u64(ctx, spill_sorted.p, ns, runs.p, run_counts.p, &cnt.p->n_runs, stream));
            hipLaunchKernelGGL(k_group_spill_emit, dim3(grid_for(ctx, ns, kChunk)), dim3(kChunk), 0, stream, runs.p, run_counts.p, &cnt.p->n_runs, need.p, only,
                               rec.p, rec_cap, &cnt.p->n_rec);
            RK_HIP(ctx, hipGetLastError());
            RK_TRY(rk_read_back(ctx, &home, cnt.p, sizeof home, stream));
            if (home.n_runs > ns) return rk_fail(ctx, RK_ERR_HIP, "rk_group_sketches: more runs than raw keys (internal error)");
            if ((again = home.n_rec > rec_cap)) rec_cap = home.n_rec;
        }
        if (!again) break;
        if (st->attempts == 2) return rk_fail(ctx, RK_ERR_HIP, "rk_group_sketches: the exact capacities overflowed (internal error)");
    }
    const unsigned long long n_rec = home.n_rec;
    if (n_rec > H) return rk_fail(ctx, RK_ERR_HIP, "rk_group_sketches: more records than postings (internal error)");

    rk_sketches *s = new (std::nothrow) rk_sketches;
    if (!s) return RK_ERR_NOMEM;
    SketchesGuard guard{s};
    s->ctx = ctx;
    s->n = K;
    s->total = n_rec;
    s->wide = idx->wide;
    RK_TRY(pool_array(ctx, &s->d_off, (size_t)K + 1));
    if (n_rec) {
        unsigned kbits = 1;
        while (kbits < 32 && (1ULL << kbits) < K) kbits++;
        RK_HIP(ctx, sorted.alloc(n_rec));
        RK_TRY(rk_prim_sort_keys_u64(ctx, rec.p, sorted.p, n_rec, 0, 32 + kbits, stream));
    }
    hipLaunchKernelGGL(k_group_offsets, dim3(blocks_for((uint64_t)K + 1)), dim3(kThreads), 0, stream, sorted.p, n_rec, K, s->d_off);
    RK_HIP(ctx, hipGetLastError());
    RK_TRY(with_hash_type(idx->wide, [&](auto ht) -> int {
        using Hash = decltype(ht);
        Hash *&hashes = hashes_of(s, ht);
        RK_TRY(pool_array(ctx, &hashes, n_rec + 1));
        const Hash *uhash;
        if constexpr (sizeof(Hash) == 8) uhash = idx->d_uhash64; else uhash = idx->d_uhash;
        if (n_rec) hipLaunchKernelGGL(k_group_hashes<Hash>, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, sorted.p, n_rec, uhash, hashes);
        RK_HIP(ctx, hipGetLastError());
        return RK_OK;
    }));
    RK_HIP(ctx, span.end());
    s->h_off.assign((size_t)K + 1, 0);
    RK_HIP(ctx, hipMemcpyAsync(s->h_off.data(), s->d_off, ((size_t)K + 1) * 8, hipMemcpyDeviceToHost, stream));
    RK_HIP(ctx, hipStreamSynchronize(stream));
    span.read();
    if (s->h_off[0] != 0 || s->h_off[K] != n_rec) return rk_fail(ctx, RK_ERR_HIP, "rk_group_sketches: the offsets of the groups do not span the records (internal error)");
    for (uint32_t g = 0; g < K; g++) {
        if (s->h_off[g + 1] < s->h_off[g]) return rk_fail(ctx, RK_ERR_HIP, "rk_group_sketches: the offsets of the groups do not ascend (internal error)");
        s->max_size = std::max<uint64_t>(s->max_size, s->h_off[g + 1] - s->h_off[g]);
    }
    s->is_set = true;   // within a group the list numbers ascend strictly, and the hashes with them
    st->block_lists = home.n_block;
    st->wave_lists = home.n_wave;
    st->lane_lists = U - home.n_wave - home.n_block;
    st->spilled = home.spilled;
    guard.p = nullptr;
    *out = s;
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_group_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, uint32_t n_genomes, const uint32_t *labels, const rk_group_rule *rule,
                   uint64_t **off_out, uint64_t **kept_out, uint32_t **group_label_out, uint32_t **group_size_out, uint32_t *n_groups)
{
    if (!rule || !off_out || !kept_out || !group_label_out || !group_size_out || !n_groups) return RK_ERR_ARG;
    if ((n_lists && !counts) || (n_genomes && !labels) || !rule_ok(rule)) return RK_ERR_ARG;
    if (n_genomes > (1u << 31)) return RK_ERR_UNSUPPORTED;
    uint64_t total = 0;
    for (uint64_t u = 0; u < n_lists; u++) total += counts[u];
    if (total && !postings) return RK_ERR_ARG;
    for (uint64_t k = 0; k < total; k++)
        if (postings[k] >= n_genomes) return RK_ERR_ARG;
    Groups gr;
    if (int rc = make_groups(labels, n_genomes, rule, &gr)) return rc;
    std::vector<uint64_t> off, kept;
    group_lists(postings, counts, n_lists, gr, rule->only, &off, &kept);
    const uint32_t K = gr.count();
    uint64_t *o = host_copy(off), *k = kept.empty() ? nullptr : host_copy(kept);
    uint32_t *gl = K ? host_copy(gr.label) : nullptr, *gs = K ? host_copy(gr.size) : nullptr;
    if (!o || (!kept.empty() && !k) || (K && (!gl || !gs))) {
        free(o);
        free(k);
        free(gl);
        free(gs);
        return RK_ERR_NOMEM;
    }
    *off_out = o;
    *kept_out = k;
    *group_label_out = gl;
    *group_size_out = gs;
    *n_groups = K;
    return RK_OK;
}

int rk_group_sketches(rk_ctx *ctx, const rk_index *idx, const uint32_t *labels, const rk_group_rule *rule, rk_sketches **out, uint32_t **group_label_out,
                      uint32_t **group_size_out, uint32_t *n_groups, rk_group_stats *stats)
{
    if (!ctx || !idx || !rule || !out || !group_label_out || !group_size_out || !n_groups) return RK_ERR_ARG;
    const uint32_t N = idx->n_ref;
    if (N && !labels) return rk_fail(ctx, RK_ERR_ARG, "rk_group_sketches: labels is null");
    if (!rule_ok(rule))
        return rk_fail(ctx, RK_ERR_ARG, "rk_group_sketches: a rule needs share_num <= share_den, share_den >= 1, min_count >= 1 and only 0 or 1");
    if (!idx->d_postings || !idx->d_upos || idx->n_shards > 1)
        return rk_fail(ctx, RK_ERR_ARG, "rk_group_sketches: an index without all posting lists (rk_index_join_shard, one hash range of a sharded build)");
    if (N > (1u << 31)) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_group_sketches: more than 2^31 genomes");
    Groups gr;
    if (make_groups(labels, N, rule, &gr)) return rk_fail(ctx, RK_ERR_ARG, "rk_group_sketches: a label is neither below the number of genomes nor RK_GROUP_NONE");
    const uint32_t K = gr.count();
    rk_group_stats st;
    memset(&st, 0, sizeof st);
    fill_constants(&st);
    st.lists = idx->U;
    st.postings = idx->H;
    st.labelled = gr.labelled;
    st.groups = K;
    const TimedSpan span{ctx, RK_MS_GROUP};
    span.clear();
    rk_sketches *s = nullptr;
    uint32_t *gl = nullptr, *gs = nullptr;
    if (K) {
        if (rk_switched_off("RK_GROUP_DEVICE")) {
            st.path = 2;
            RK_TRY(idx->wide ? group_on_host<uint64_t>(ctx, idx, gr, rule->only, &s) : group_on_host<uint32_t>(ctx, idx, gr, rule->only, &s));
        } else {
            st.path = 1;
            RK_TRY(group_on_device(ctx, idx, gr, rule->only, &st, &s));
        }
        st.kept = s->total;
        gl = host_copy(gr.label);
        gs = host_copy(gr.size);
        if (!gl || !gs) {
            free(gl);
            free(gs);
            rk_sketches_free(s);
            return rk_fail(ctx, RK_ERR_NOMEM, "rk_group_sketches: out of host memory");
        }
    }
    *out = s;
    *group_label_out = gl;
    *group_size_out = gs;
    *n_groups = K;
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
