// rk_lca.hip -- query sketches classified by the per-hash lowest common ancestor in a taxonomy over the references (rk_lca_rows), the same
// rule on the host over exported lists (rk_lca_lists) and the call on a tally (rk_lca_call).  parent[t] == t is the one root; taxa[v] names
// the node of reference v (RK_LCA_NONE: unlabelled).  lca(h) = the LCA of the taxa of the labelled holders of h; a query row is the tally
// of lca over its matched ELEMENTS: {taxon, direct} by ascending node id, plus matched and unlabelled.  include/rabbitkssd.h, taxonomic
// classification by per-hash LCA.
//
//   host      the taxonomy validated (one root, parents in range, no cycle: a colouring walk, no recursion) and numbered in preorder by an
//             iterative DFS, children by ascending id.  Uploaded once: per preorder id its parent, the last preorder id of its subtree and
//             its node; per node its preorder id; taxa: 16 T + 4 N bytes;
//   taxa      k_lca_taxa: the preorder id of every genome's taxon in INTERNAL genome order through d_orig (an imported index: taxa itself);
//   lists     in preorder a subtree is an interval, so the LCA of a set is the LCA of its members with the smallest and the largest
//             preorder id: a list needs an integer min and max over its labelled postings (order-free, exact) and ONE climb,
//             a = min; while (last[a] < max) a = parent[a].  By the length of a list, as rk_group.hip splits them:
//             k_lca_lane   up to kLaneMax postings: one lane per list, all postings loaded first, then all their taxa; the same sweep
//                          queues the longer lists (one wave-aggregated reservation per queue);
//             k_lca_wave   up to kWaveMax: one wave per list, kWavePer postings per lane, kWaveBatch lists per trip so that their loads
//                          are in flight together; min and max across the lanes by shuffles; lane j climbs for list j of the batch;
//             k_lca_block  longer lists: one workgroup per list streams chunks of kChunk postings (kChunkPer per thread), min and max
//                          reduced across the waves through LDS; thread 0 climbs;
//             list_taxon[U] holds the CALLER's node id of lca(h), kUnlabelled for a list without a labelled holder;
//   tally     k_lca_tally: flat over ALL query elements in tiles of kTileHashes, whatever sketch they belong to.  Per element the look-up
//             (rk_query_dev.h), list_taxon, and its row: a binary search among the query offsets for the last row that starts at or
//             before it (runs of empty sketches fall out).  Elements of unselected rows emit nothing.  The equal keys row << 32 | taxon
//             of a run of 64 elements are counted by ballots, then added to an LDS table of kTableSlots slots (64-bit compare-and-swap on
//             the key, an add on the count): more slots than a tile has elements, it cannot overflow.  Then ONE reservation per tile and
//             the table's (key, count) pairs go to the partial records.  unlabelled travels under the reserved taxon kUnlabelled;
//   overflow  the counter keeps counting past the capacity; the tally then runs once more with the exact count (attempts = 2);
//   fold      rk_prim_sort_pairs_u64_u32 over the bits in use; k_lca_fold_flag marks the first partial of every key with a real taxon,
//             an inclusive scan numbers the records; k_lca_fold_sum, one lane per run of equal keys (a run is at most the tiles a row
//             spans), writes the record or unlabelled[row] and adds the run to matched[row]; k_lca_fold_offsets, one lane per offset
//             entry, a lower bound among the sorted keys: Q + 1 offsets.
//
// Memory scope: every array is written by one kernel and read by a later one on the same stream.  INSIDE a launch the only communication
// between workgroups is relaxed agent-scope adds (and one max) on counters and on matched[], which nobody reads before the launch is over;
// inside k_lca_tally and k_lca_block LDS atomics between barriers.  No loop waits for another workgroup: any grid works.  The host
// synchronises for the counters before the sort, for offsets + per-row counts, and for the records.  DESIGN.md 4.17.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "rk_internal.h"
#include "rk_query_dev.h"
#include "rk_query_host.h"

namespace {

constexpr uint32_t kNone = RK_LCA_NONE;
constexpr uint32_t kUnlabelled = 0x80000000u;   // list_taxon / the taxon of a key: no labelled holder (node ids lie below 2^31)
constexpr int kLaneMax = 32;                    // k_lca_lane: the longest list one lane takes (8 / 12 / 16 / 32 measured: DESIGN.md 4.17)
constexpr int kWavePer = 4, kWaveMax = 64 * kWavePer;   // k_lca_wave: postings per lane, the longest list one wave takes
constexpr int kWaveBatch = 4;                   // lists of one trip of k_lca_wave
constexpr int kLcaThreads = 256;                // threads of every workgroup of this unit: 4 waves
constexpr int kChunkPer = 4, kChunk = kLcaThreads * kChunkPer;   // k_lca_block: postings per thread and per chunk
constexpr int kTrips = 8;                       // runs of 64 elements one wave takes of a tile
constexpr int kTileHashes = kLcaThreads * kTrips;   // 2048
constexpr int kTableBits = 12, kTableSlots = 1 << kTableBits;
constexpr int kSlotsPer = kTableSlots / kLcaThreads;
constexpr unsigned long long kEmpty = ~0ULL;    // (no key: a row lies below 2^32 - 1)
static_assert(kTableSlots > kTileHashes, "the table has room for every element of a tile as a key of its own: it cannot overflow");
static_assert(kTableSlots % kLcaThreads == 0 && kTableSlots * 12 <= 64 * 1024, "a thread flushes kSlotsPer slots; keys and counts fit the LDS of a workgroup");
static_assert(kWaveBatch <= 64 && 64 % kWaveBatch == 0 && kLaneMax < kWaveMax && kWaveMax < kChunk, "the classes of list lengths");
static_assert(sizeof(rk_lca_opts) == 12 && sizeof(rk_lca_count) == 8 && sizeof(rk_lca_rule) == 16 && sizeof(rk_lca_called) == 24 &&
              sizeof(rk_lca_stats) == 128, "the layouts of include/rabbitkssd.h");

struct Counters {   // one device block, read back in one copy
    unsigned long long n_wave, n_block, partials;
    uint32_t longest, pad_;
};

struct ListArgs {
    const uint32_t *postings, *upos;          // the index: u32[H], u32[U + 1]
    const uint32_t *gtax;                     // preorder id of the taxon per INTERNAL genome id (kNone: unlabelled)
    const uint32_t *ppar, *last, *node_of;    // per preorder id: its parent's, the last of its subtree, the caller's node
    unsigned long long U;
    uint32_t *list_taxon;                     // u32[U]
    uint32_t *wave_q, *block_q;               // the lists of the two longer classes
    Counters *cnt;
};

struct TallyArgs {
    const void *q_hashes;              // Hash[total]
    const uint64_t *q_off;             // u64[n + 1]
    unsigned long long total;
    uint32_t n;
    IndexLookup ix;
    const uint32_t *list_taxon;
    uint32_t row_first, row_step, row_block;   // (step and block at least 1)
    unsigned long long *part_key, cap;         // row << 32 | taxon
    uint32_t *part_cnt;
    Counters *cnt;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
// the preorder ids of the genomes' taxa in the index's internal genome order
__global__ void k_lca_taxa(const uint32_t *taxa, const uint32_t *pre, const uint32_t *orig, uint32_t n, uint32_t *gtax)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = taxa[orig ? orig[i] : i];   // (orig[] < n: rk_index_build's permutation; t < T or kNone: the host checked)
    gtax[i] = t == kNone ? kNone : pre[t];
}

// mn / mx: the smallest and the largest preorder id among the labelled postings of list u (mn == kNone: none is labelled).  One climb
// from mn to the first ancestor whose subtree reaches mx (the root's reaches T - 1 >= mx: the loop ends); returns its steps.
__device__ __forceinline__ uint32_t climb_store(const ListArgs &a, unsigned long long u, uint32_t mn, uint32_t mx)
{
    if (mn == kNone) {
        a.list_taxon[u] = kUnlabelled;
        return 0;
    }
    uint32_t at = mn, steps = 0;
    while (a.last[at] < mx) {
        at = a.ppar[at];
        steps++;
    }
    a.list_taxon[u] = a.node_of[at];
    return steps;
}
__device__ __forceinline__ void report_climb(const ListArgs &a, uint32_t steps)
{
    const uint32_t m = wave_max(steps);
    if ((threadIdx.x & 63) == 0 && m) __hip_atomic_fetch_max(&a.cnt->longest, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per list; the lists of up to kLaneMax postings are decided here, the longer ones queued (wave_q has room for every list of
// more than kLaneMax postings, block_q for every list of more than kWaveMax: the host sized them from H).  All postings first (a slot
// beyond the list reads posting 0 and is masked afterwards), then all taxa: two round trips per list.
__global__ void __launch_bounds__(kLcaThreads) k_lca_lane(ListArgs a)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long wave = ((unsigned long long)blockIdx.x * kLcaThreads + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * (kLcaThreads / 64);
    uint32_t longest = 0;
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
        uint32_t p[kLaneMax], g[kLaneMax];
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) p[j] = a.postings[(uint32_t)j < mine_len ? beg + j : 0u];   // (U > 0: posting 0 exists)
#pragma unroll
        for (int j = 0; j < kLaneMax; j++) g[j] = a.gtax[p[j]];
        uint32_t mn = kNone, mx = 0;
#pragma unroll
        for (int j = 0; j < kLaneMax; j++)
            if ((uint32_t)j < mine_len && g[j] != kNone) {
                mn = min(mn, g[j]);
                mx = max(mx, g[j]);
            }
        if (u < a.U && len <= (uint32_t)kLaneMax) longest = max(longest, climb_store(a, u, mn, mx));
    }
    report_climb(a, longest);
}

// One wave per queued list of kLaneMax < len <= kWaveMax postings, kWaveBatch lists per trip: lane l reads postings l, l + 64, .. of each.
__global__ void __launch_bounds__(kLcaThreads) k_lca_wave(ListArgs a)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long wave = ((unsigned long long)blockIdx.x * kLcaThreads + threadIdx.x) >> 6, n_waves = (unsigned long long)gridDim.x * (kLcaThreads / 64);
    const unsigned long long n = a.cnt->n_wave;   // (final: k_lca_lane is through)
    uint32_t longest = 0;
    for (unsigned long long first = wave * 64; first < n; first += n_waves * 64) {   // (uniform per wave)
        uint32_t u_l = 0, beg_l = 0, len_l = 0;   // lane l: queue entry first + l (len 0 beyond the queue)
        if (first + lane < n) {
            u_l = a.wave_q[first + lane];
            beg_l = a.upos[u_l];
            len_l = a.upos[u_l + 1] - beg_l;
        }
        const int here = (int)(n - first < 64 ? n - first : 64);
        for (int k0 = 0; k0 < here; k0 += kWaveBatch) {   // (uniform; k0 + kWaveBatch <= 64)
            uint32_t p[kWaveBatch][kWavePer], g[kWaveBatch][kWavePer];
            bool valid[kWaveBatch][kWavePer];
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) {
                const uint32_t beg = (uint32_t)__shfl((int)beg_l, k0 + j), len = (uint32_t)__shfl((int)len_l, k0 + j);
#pragma unroll
                for (int k = 0; k < kWavePer; k++) {
                    valid[j][k] = (uint32_t)(64 * k + lane) < len;
                    p[j][k] = a.postings[valid[j][k] ? beg + 64 * k + lane : 0u];
                }
            }
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++)
#pragma unroll
                for (int k = 0; k < kWavePer; k++) g[j][k] = a.gtax[p[j][k]];
            uint32_t my_mn = kNone, my_mx = 0, my_u = 0;
            bool climbs = false;
#pragma unroll
            for (int j = 0; j < kWaveBatch; j++) {
                uint32_t mn = kNone, mx = 0;
#pragma unroll
                for (int k = 0; k < kWavePer; k++)
                    if (valid[j][k] && g[j][k] != kNone) {
                        mn = min(mn, g[j][k]);
                        mx = max(mx, g[j][k]);
                    }
                mn = wave_min(mn);
                mx = wave_max(mx);
                const uint32_t u = (uint32_t)__shfl((int)u_l, k0 + j);
                if (lane == j) {   // lane j climbs for list j of the batch
                    my_mn = mn;
                    my_mx = mx;
                    my_u = u;
                    climbs = k0 + j < here;
                }
            }
            if (climbs) longest = max(longest, climb_store(a, my_u, my_mn, my_mx));
        }
    }
    report_climb(a, longest);
}

// One workgroup per queued list of more than kWaveMax postings, streamed in chunks of kChunk
__global__ void __launch_bounds__(kLcaThreads) k_lca_block(ListArgs a)
{
    __shared__ uint32_t s_mn[kLcaThreads / 64], s_mx[kLcaThreads / 64];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long n = a.cnt->n_block;   // (final: k_lca_lane is through)
    uint32_t longest = 0;
    for (unsigned long long i = blockIdx.x; i < n; i += gridDim.x) {   // (uniform per workgroup)
        const uint32_t u = a.block_q[i];
        const uint32_t beg = a.upos[u], len = a.upos[u + 1] - beg;
        uint32_t mn = kNone, mx = 0;
        for (uint32_t base = 0; base < len; base += kChunk) {   // (uniform)
            uint32_t p[kChunkPer], g[kChunkPer];
#pragma unroll
            for (int k = 0; k < kChunkPer; k++) {
                const uint32_t at = base + (uint32_t)k * kLcaThreads + tid;
                p[k] = a.postings[at < len ? beg + at : beg];
            }
#pragma unroll
            for (int k = 0; k < kChunkPer; k++) g[k] = a.gtax[p[k]];
#pragma unroll
            for (int k = 0; k < kChunkPer; k++)
                if (base + (uint32_t)k * kLcaThreads + tid < len && g[k] != kNone) {
                    mn = min(mn, g[k]);
                    mx = max(mx, g[k]);
                }
        }
        mn = wave_min(mn);
        mx = wave_max(mx);
        if (lane == 0) {
            s_mn[wave] = mn;
            s_mx[wave] = mx;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 0; w < kLcaThreads / 64; w++) {
                mn = min(mn, s_mn[w]);
                mx = max(mx, s_mx[w]);
            }
            longest = max(longest, climb_store(a, u, mn, mx));
        }
        __syncthreads();   // (s_mn / s_mx are free for the next list)
    }
    report_climb(a, longest);
}

__device__ __forceinline__ uint32_t table_slot(unsigned long long key)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ULL) >> (64 - kTableBits));
}

template <class Hash> __global__ void __launch_bounds__(kLcaThreads) k_lca_tally(TallyArgs a)
{
    __shared__ unsigned long long s_key[kTableSlots];
    __shared__ uint32_t s_cnt[kTableSlots];
    __shared__ uint32_t s_wave[kLcaThreads / 64];
    __shared__ unsigned long long s_base;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    for (uint32_t s = tid; s < (uint32_t)kTableSlots; s += kLcaThreads) {
        s_key[s] = kEmpty;
        s_cnt[s] = 0;
    }
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * kTileHashes + (unsigned long long)wave * (kTrips * 64);
    const Hash *q = (const Hash *)a.q_hashes;
    unsigned long long h[kTrips], key[kTrips];
    bool in[kTrips], mine[kTrips];
    uint32_t list[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const unsigned long long j = base + 64 * t + lane;
        in[t] = j < a.total;
        h[t] = in[t] ? (unsigned long long)q[j] : 0ULL;
    }
    index_lookup<Hash, kTrips>(a.ix, h, in, list);
    uint32_t tx[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) tx[t] = list[t] != kNoList ? a.list_taxon[list[t]] : 0u;
    // the row of a matched element j: the last r with q_off[r] <= j (j < total = q_off[n]: r < n); the searches of a lane advance together
    unsigned long long rlo[kTrips], rhi[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        rlo[t] = 0;
        rhi[t] = list[t] != kNoList ? a.n : 0ULL;
    }
    for (bool more = true; more;) {
        more = false;
#pragma unroll
        for (int t = 0; t < kTrips; t++)
            if (rlo[t] < rhi[t]) {
                const unsigned long long mid = (rlo[t] + rhi[t] + 1) >> 1;   // (1 <= mid <= n)
                if (a.q_off[mid] <= base + 64 * t + lane) rlo[t] = mid; else rhi[t] = mid - 1;
                more |= rlo[t] < rhi[t];
            }
    }
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const uint32_t blk = (uint32_t)rlo[t] / a.row_block;
        mine[t] = list[t] != kNoList && blk >= a.row_first && (blk - a.row_first) % a.row_step == 0;
        key[t] = (rlo[t] << 32) | tx[t];
    }
    // the equal keys of a run of 64 elements are counted by ballots (one round per distinct key: neighbours share row and, mostly, taxon),
    // then the first lane of every key adds its count to the table
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        unsigned long long pending = __ballot(mine[t]);
        uint32_t c = 0;
        while (pending) {   // (uniform)
            const int lead = __ffsll((long long)pending) - 1;
            const unsigned long long kl = shfl_u64(key[t], lead);
            const unsigned long long m = __ballot(mine[t] && key[t] == kl);
            if (lane == lead) c = (uint32_t)__popcll(m);
            pending &= ~m;
        }
        if (c) {
            // at most kTileHashes < kTableSlots keys: a free slot exists
            uint32_t slot = table_slot(key[t]);
            for (int probe = 0; probe < kTableSlots; probe++) {
                const unsigned long long old = atomicCAS(&s_key[slot], kEmpty, key[t]);
                if (old == kEmpty || old == key[t]) {
                    atomicAdd(&s_cnt[slot], c);
                    break;
                }
                slot = (slot + 1) & (kTableSlots - 1);
            }
        }
    }
    __syncthreads();
    // one reservation per tile: thread i flushes slots i, i + 256, ..
    uint32_t n_mine = 0;
#pragma unroll
    for (int k = 0; k < kSlotsPer; k++) n_mine += s_key[k * kLcaThreads + tid] != kEmpty;
    uint32_t incl = n_mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kLcaThreads / 64; w++) {
        if (w < wave) before += s_wave[w];
        sum += s_wave[w];
    }
    if (!sum) return;   // (uniform: nothing of this tile is matched and selected)
    if (tid == 0) s_base = add_u64(&a.cnt->partials, sum);
    __syncthreads();
    unsigned long long at = s_base + before + incl - n_mine;
#pragma unroll
    for (int k = 0; k < kSlotsPer; k++) {
        const unsigned long long kk = s_key[k * kLcaThreads + tid];
        if (kk != kEmpty) {
            if (at < a.cap) {
                a.part_key[at] = kk;
                a.part_cnt[at] = s_cnt[k * kLcaThreads + tid];
            }
            at++;
        }
    }
}

// flag[i] = 1 for the first partial of a key with a real taxon (a record), 0 otherwise
__global__ void __launch_bounds__(kLcaThreads) k_lca_fold_flag(const unsigned long long *key, unsigned long long n, uint32_t *flag)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kLcaThreads + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || key[i - 1] != key[i]) && (uint32_t)key[i] < kUnlabelled;
}

// one lane per run of equal keys: its sum becomes a record (rank = the inclusive scan of the flags) or unlabelled[row]; matched[row] adds it
__global__ void __launch_bounds__(kLcaThreads) k_lca_fold_sum(const unsigned long long *key, const uint32_t *cnt, const uint32_t *rank, unsigned long long n,
                                                             rk_lca_count *rec, uint32_t *matched, uint32_t *unlabelled)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kLcaThreads + threadIdx.x;
    if (i >= n || (i > 0 && key[i - 1] == key[i])) return;
    const unsigned long long k = key[i];
    uint32_t sum = 0;   // (a row has fewer than 2^32 elements)
    for (unsigned long long j = i; j < n && key[j] == k; j++) sum += cnt[j];
    const uint32_t row = (uint32_t)(k >> 32), tx = (uint32_t)k;
    if (tx == kUnlabelled) unlabelled[row] = sum;
    else rec[rank[i] - 1] = rk_lca_count{tx, sum};   // (rank[i] >= 1: partial i is flagged; rank <= n)
    __hip_atomic_fetch_add(&matched[row], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// off[g] = the records of the rows before g, g = 0 .. Q
__global__ void __launch_bounds__(kLcaThreads) k_lca_fold_offsets(const unsigned long long *key, const uint32_t *rank, unsigned long long n, uint32_t Q, uint64_t *off)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * kLcaThreads + threadIdx.x;
    if (g > Q) return;
    unsigned long long lo = 0, hi = n;   // the partials of rows below g
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if ((key[mid] >> 32) < g) lo = mid + 1; else hi = mid;
    }
    off[g] = lo ? rank[lo - 1] : 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
unsigned long long env_number(const char *name, unsigned long long dflt)
{
    const char *s = getenv(name);
    return s && *s ? strtoull(s, nullptr, 10) : dflt;
}

// The taxonomy, checked: RK_OK and depth[] (the root's is 0), or RK_ERR_ARG.  A colouring walk towards the root: a node is open while
// the walk that found it is under way; meeting an open node is a cycle.  No recursion.
int check_taxonomy(const uint32_t *parent, uint32_t T, std::vector<uint32_t> *depth, uint32_t *root_out)
{
    if (!parent || !T) return RK_ERR_ARG;
    if (T >= 0x80000000u) return RK_ERR_UNSUPPORTED;
    uint32_t root = kNone;
    for (uint32_t t = 0; t < T; t++) {
        if (parent[t] >= T) return RK_ERR_ARG;
        if (parent[t] == t) {
            if (root != kNone) return RK_ERR_ARG;
            root = t;
        }
    }
    if (root == kNone) return RK_ERR_ARG;
    std::vector<unsigned char> state(T, 0);   // 0 new, 1 open, 2 done
    depth->assign(T, 0);
    state[root] = 2;
    std::vector<uint32_t> path;
    for (uint32_t t = 0; t < T; t++) {
        uint32_t at = t;
        path.clear();
        while (state[at] == 0) {
            state[at] = 1;
            path.push_back(at);
            at = parent[at];
        }
        if (state[at] == 1) return RK_ERR_ARG;   // a cycle
        uint32_t d = (*depth)[at];
        for (size_t k = path.size(); k-- > 0;) {
            (*depth)[path[k]] = ++d;
            state[path[k]] = 2;
        }
    }
    *root_out = root;
    return RK_OK;
}

int check_taxa(const uint32_t *taxa, uint32_t N, uint32_t T)
{
    if (N && !taxa) return RK_ERR_ARG;
    for (uint32_t v = 0; v < N; v++)
        if (taxa[v] >= T && taxa[v] != kNone) return RK_ERR_ARG;
    return RK_OK;
}

// the LCA of two nodes by depth and parent steps (the host leg's; the device leg numbers in preorder instead)
inline uint32_t lca2(const uint32_t *parent, const uint32_t *depth, uint32_t a, uint32_t b)
{
    while (depth[a] > depth[b]) a = parent[a];
    while (depth[b] > depth[a]) b = parent[b];
    while (a != b) {
        a = parent[a];
        b = parent[b];
    }
    return a;
}

struct Preorder {   // per preorder id: parent, last of the subtree, node; per node: preorder id
    std::vector<uint32_t> ppar, last, node_of, pre;
};

// an iterative DFS from the root, children by ascending id (a counting sort by parent keeps them so)
void number_preorder(const uint32_t *parent, uint32_t T, uint32_t root, Preorder *po)
{
    std::vector<uint32_t> first((size_t)T + 1, 0), child(T ? T - 1 : 0), next_child(T);
    for (uint32_t t = 0; t < T; t++)
        if (t != root) first[parent[t] + 1]++;
    for (uint32_t t = 0; t < T; t++) first[t + 1] += first[t];
    {
        std::vector<uint32_t> fill(first.begin(), first.end() - 1);
        for (uint32_t t = 0; t < T; t++)
            if (t != root) child[fill[parent[t]]++] = t;
    }
    po->ppar.assign(T, 0);
    po->last.assign(T, 0);
    po->node_of.assign(T, 0);
    po->pre.assign(T, 0);
    for (uint32_t t = 0; t < T; t++) next_child[t] = first[t];
    std::vector<uint32_t> stack;
    uint32_t n = 0;
    po->pre[root] = n;
    po->node_of[n] = root;
    po->ppar[n] = n;
    n++;
    stack.push_back(root);
    while (!stack.empty()) {
        const uint32_t t = stack.back();
        if (next_child[t] < first[t + 1]) {
            const uint32_t c = child[next_child[t]++];
            po->pre[c] = n;
            po->node_of[n] = c;
            po->ppar[n] = po->pre[t];
            n++;
            stack.push_back(c);
        } else {
            po->last[po->pre[t]] = n - 1;
            stack.pop_back();
        }
    }
}

void fill_constants(rk_lca_stats *st, uint64_t all_elements)
{
    st->lane_max = kLaneMax;
    st->wave_max = kWaveMax;
    st->chunk = kChunk;
    st->tile_hashes = kTileHashes;
    st->table_slots = kTableSlots;
    st->threads = kLcaThreads;
    st->tiles = (all_elements + kTileHashes - 1) / kTileHashes;
}

struct HostResult {
    std::vector<rk_lca_count> recs;
    std::vector<uint64_t> off;                    // Q + 1
    std::vector<uint32_t> matched, unlabelled;    // Q (unselected rows: 0)
};

// The rule over lists: list u is postings[pos[u] .. pos[u + 1]); per query the lists of its matched elements.  lca(list) is folded pairwise.
void lca_core(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off, const uint64_t *q_lists, uint32_t Q,
              const uint32_t *taxa, const uint32_t *parent, const uint32_t *depth, const RowSel &sel, HostResult *out, rk_lca_stats *st)
{
    std::vector<uint32_t> list_taxon(n_lists, kNone);
    uint64_t pos = 0;
    for (uint64_t u = 0; u < n_lists; u++) {
        uint32_t l = kNone;
        for (uint64_t k = pos; k < pos + counts[u]; k++) {
            const uint32_t t = taxa[postings[k]];
            if (t != kNone) l = l == kNone ? t : lca2(parent, depth, l, t);
        }
        list_taxon[u] = l;
        pos += counts[u];
        if (counts[u] <= (uint32_t)kLaneMax) st->lane_lists++;
        else if (counts[u] <= (uint32_t)kWaveMax) st->wave_lists++;
        else st->block_lists++;
    }
    st->lists = n_lists;
    st->postings = pos;
    out->off.assign((size_t)Q + 1, 0);
    out->matched.assign(Q, 0);
    out->unlabelled.assign(Q, 0);
    out->recs.clear();
    std::vector<uint32_t> seen;
    size_t next = 0;
    for (uint32_t q = 0; q < Q; q++) {
        if (next < sel.rows.size() && sel.rows[next] == q) {
            next++;
            seen.clear();
            for (uint64_t j = q_off[q]; j < q_off[q + 1]; j++) {
                const uint32_t t = list_taxon[q_lists[j]];
                if (t == kNone) out->unlabelled[q]++;
                else seen.push_back(t);
            }
            out->matched[q] = (uint32_t)(q_off[q + 1] - q_off[q]);
            std::sort(seen.begin(), seen.end());
            for (size_t k = 0; k < seen.size();) {
                size_t e = k;
                while (e < seen.size() && seen[e] == seen[k]) e++;
                out->recs.push_back(rk_lca_count{seen[k], (uint32_t)(e - k)});
                k = e;
            }
            st->matched += out->matched[q];
            st->unlabelled += out->unlabelled[q];
        }
        out->off[q + 1] = out->recs.size();
    }
    st->records = out->recs.size();
}

using Result = RowsResult<rk_lca_count, 2>;   // per row: matched, unlabelled

Result view(const HostResult &r)
{
    return Result{r.off.data(), {r.matched.data(), r.unlabelled.data()}, r.recs.data(), r.recs.size()};
}

// RK_LCA_DEVICE=0: export + the lists of the selected rows' elements (a binary search each) + the rule over lists
template <class Hash>
int lca_on_host(rk_ctx *ctx, const rk_index *idx, const rk_sketches *qs, const uint32_t *taxa, const uint32_t *parent, const uint32_t *depth, const RowSel &sel,
                HostResult *out, rk_lca_stats *st)
{
    const uint32_t Q = qs->n;
    std::vector<uint32_t> postings(idx->H), counts(idx->U);
    std::vector<Hash> hashes(idx->U), qh(qs->total);
    std::vector<uint64_t> qoff((size_t)Q + 1);
    if constexpr (sizeof(Hash) == 8) {
        if (idx->U) RK_TRY(rk_index_export64(idx, postings.data(), hashes.data(), counts.data()));
        RK_TRY(rk_sketches_download64(qs, qh.data(), qoff.data()));
    } else {
        if (idx->U) RK_TRY(rk_index_export_lists(idx, postings.data(), hashes.data(), counts.data()));
        RK_TRY(rk_sketches_download(qs, qh.data(), qoff.data()));
    }
    for (const uint32_t p : postings)
        if (p >= idx->n_ref) return rk_fail(ctx, RK_ERR_HIP, "rk_lca_rows: an exported posting names a genome beyond their number (internal error)");
    std::vector<uint64_t> l_off((size_t)Q + 1, 0), l;
    size_t next = 0;
    for (uint32_t q = 0; q < Q; q++) {
        if (next < sel.rows.size() && sel.rows[next] == q) {
            next++;
            // (a hash at or beyond 2^hash_bits is none of the exported hashes: the index holds none)
            for (uint64_t j = qoff[q]; j < qoff[q + 1]; j++) {
                const auto it = std::lower_bound(hashes.begin(), hashes.end(), qh[j]);
                if (it != hashes.end() && *it == qh[j]) l.push_back((uint64_t)(it - hashes.begin()));
            }
        }
        l_off[q + 1] = l.size();
    }
    lca_core(postings.data(), counts.data(), idx->U, l_off.data(), l.data(), Q, taxa, parent, depth, sel, out, st);
    return RK_OK;
}

struct DeviceResult {
    std::vector<unsigned char> head;   // Result::from_block without the records
    std::vector<rk_lca_count> recs;
};

int lca_on_device(rk_ctx *ctx, const rk_index *idx, const rk_sketches *qs, const uint32_t *taxa, const uint32_t *parent, uint32_t T, uint32_t root,
                  const rk_lca_opts *o, rk_lca_stats *st, DeviceResult *res)
{
    const uint32_t N = idx->n_ref, Q = qs->n;
    const uint64_t U = idx->U, H = idx->H, total = qs->total, tiles = st->tiles;
    if (tiles > 0x7FFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_lca_rows: more than 2^31 tiles of query elements");
    Preorder po;
    number_preorder(parent, T, root, &po);
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const TimedSpan span{ctx, RK_MS_LCA};
    RK_TRY(rk_index_ensure_dir(ctx, const_cast<rk_index *>(idx), stream));
    const uint64_t wave_cap = std::min<uint64_t>(U, H / (kLaneMax + 1) + 1), block_cap = std::min<uint64_t>(U, H / (kWaveMax + 1) + 1);
    const size_t head_bytes = Result::head_bytes(Q);
    DevBuf<uint32_t> d_tax(ctx), d_taxa(ctx), gtax(ctx), list_taxon(ctx), wave_q(ctx), block_q(ctx);
    DevBuf<Counters> cnt(ctx);
    DevBuf<unsigned char> head(ctx);
    RK_HIP(ctx, d_tax.alloc((size_t)T * 4));   // ppar | last | node_of | pre
    RK_HIP(ctx, d_taxa.alloc(N));
    RK_HIP(ctx, gtax.alloc(N));
    RK_HIP(ctx, list_taxon.alloc(U));
    RK_HIP(ctx, wave_q.alloc(wave_cap));
    RK_HIP(ctx, block_q.alloc(block_cap));
    RK_HIP(ctx, cnt.alloc(1));
    RK_HIP(ctx, head.alloc(head_bytes));
    // (pageable memory of this function: the stream is synchronised before it returns)
    RK_HIP(ctx, hipMemcpyAsync(d_tax.p, po.ppar.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemcpyAsync(d_tax.p + T, po.last.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemcpyAsync(d_tax.p + 2 * (size_t)T, po.node_of.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemcpyAsync(d_tax.p + 3 * (size_t)T, po.pre.data(), (size_t)T * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemcpyAsync(d_taxa.p, taxa, (size_t)N * 4, hipMemcpyHostToDevice, stream));
    RK_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(Counters), stream));
    RK_HIP(ctx, hipMemsetAsync(head.p, 0, head_bytes, stream));

    ListArgs la;
    memset(&la, 0, sizeof la);
    la.postings = idx->d_postings;
    la.upos = idx->d_upos;
    la.gtax = gtax.p;
    la.ppar = d_tax.p;
    la.last = d_tax.p + T;
    la.node_of = d_tax.p + 2 * (size_t)T;
    la.U = U;
    la.list_taxon = list_taxon.p;
    la.wave_q = wave_q.p;
    la.block_q = block_q.p;
    la.cnt = cnt.p;
    const unsigned wide_grid = (unsigned)std::max(1, ctx->num_cu) * 8;
    RK_HIP(ctx, span.begin());
    hipLaunchKernelGGL(k_lca_taxa, dim3(blocks_for(N)), dim3(kThreads), 0, stream, d_taxa.p, d_tax.p + 3 * (size_t)T, idx->d_orig, N, gtax.p);
    hipLaunchKernelGGL(k_lca_lane, dim3(std::min(blocks_for(U, kLcaThreads), wide_grid)), dim3(kLcaThreads), 0, stream, la);
    hipLaunchKernelGGL(k_lca_wave, dim3(std::max(1u, std::min(blocks_for(wave_cap, kLcaThreads / 64), wide_grid))), dim3(kLcaThreads), 0, stream, la);
    hipLaunchKernelGGL(k_lca_block, dim3(std::max(1u, (unsigned)std::min<uint64_t>(block_cap, wide_grid))), dim3(kLcaThreads), 0, stream, la);
    RK_HIP(ctx, hipGetLastError());

    TallyArgs ta;
    memset(&ta, 0, sizeof ta);
    ta.q_hashes = qs->wide ? (const void *)qs->d_hashes64 : (const void *)qs->d_hashes;
    ta.q_off = qs->d_off;
    ta.total = total;
    ta.n = Q;
    ta.ix = index_lookup_of(idx);
    ta.list_taxon = list_taxon.p;
    ta.row_first = o->row_first;
    ta.row_step = o->row_step ? o->row_step : 1;
    ta.row_block = o->row_block ? o->row_block : 1;
    ta.cnt = cnt.p;
    // a tile emits at most one partial per element; a genome's hashes map to a few dozen taxa
    uint64_t cap = std::min<uint64_t>(total, std::max<uint64_t>(1ULL << 20, tiles * 128));
    cap = std::max<uint64_t>(1, std::min<uint64_t>(total, env_number("RK_LCA_CAP", cap)));
    DevBuf<unsigned long long> part_key(ctx), sorted_key(ctx);
    DevBuf<uint32_t> part_cnt(ctx), sorted_cnt(ctx), rank(ctx);
    Counters home;
    memset(&home, 0, sizeof home);
    for (st->attempts = 1;; st->attempts++) {
        RK_HIP(ctx, part_key.alloc(cap));
        RK_HIP(ctx, part_cnt.alloc(cap));
        ta.part_key = part_key.p;
        ta.part_cnt = part_cnt.p;
        ta.cap = cap;
        if (tiles) {
            if (qs->wide) hipLaunchKernelGGL(k_lca_tally<uint64_t>, dim3((unsigned)tiles), dim3(kLcaThreads), 0, stream, ta);
            else hipLaunchKernelGGL(k_lca_tally<uint32_t>, dim3((unsigned)tiles), dim3(kLcaThreads), 0, stream, ta);
            RK_HIP(ctx, hipGetLastError());
        }
        RK_TRY(rk_read_back(ctx, &home, cnt.p, sizeof home, stream));
        if (home.partials <= cap) break;
        if (st->attempts == 2 || home.partials > total) return rk_fail(ctx, RK_ERR_HIP, "rk_lca_rows: the partial records outgrew their exact count (internal error)");
        cap = home.partials;
        RK_HIP(ctx, hipMemsetAsync(&cnt.p->partials, 0, 8, stream));
    }
    const uint64_t n_part = home.partials;
    if (n_part >= 0xFFFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_lca_rows: 2^32 - 1 partial records or more");
    if (home.n_wave > wave_cap || home.n_block > block_cap) return rk_fail(ctx, RK_ERR_HIP, "rk_lca_rows: more long lists than postings allow (internal error)");
    uint64_t *d_off = (uint64_t *)head.p;
    uint32_t *d_matched = (uint32_t *)(head.p + ((size_t)Q + 1) * 8), *d_unl = d_matched + Q;
    DevBuf<rk_lca_count> rec(ctx);
    if (n_part) {
        unsigned row_bits = 1;
        while (row_bits < 32 && (1ULL << row_bits) < Q) row_bits++;
        RK_HIP(ctx, sorted_key.alloc(n_part));
        RK_HIP(ctx, sorted_cnt.alloc(n_part));
        RK_HIP(ctx, rank.alloc(n_part));
        RK_HIP(ctx, rec.alloc(n_part));
        RK_TRY(rk_prim_sort_pairs_u64_u32(ctx, (const uint64_t *)part_key.p, (uint64_t *)sorted_key.p, part_cnt.p, sorted_cnt.p, n_part, 32 + row_bits, stream));
        const unsigned pb = blocks_for(n_part, kLcaThreads);
        hipLaunchKernelGGL(k_lca_fold_flag, dim3(pb), dim3(kLcaThreads), 0, stream, sorted_key.p, n_part, part_cnt.p);   // (part_cnt is free: the flags)
        RK_HIP(ctx, hipGetLastError());
        RK_TRY(rk_prim_inclusive_scan_u32(ctx, part_cnt.p, rank.p, n_part, stream));
        hipLaunchKernelGGL(k_lca_fold_sum, dim3(pb), dim3(kLcaThreads), 0, stream, sorted_key.p, sorted_cnt.p, rank.p, n_part, rec.p, d_matched, d_unl);
        hipLaunchKernelGGL(k_lca_fold_offsets, dim3(blocks_for((uint64_t)Q + 1, kLcaThreads)), dim3(kLcaThreads), 0, stream, sorted_key.p, rank.p, n_part, Q, d_off);
        RK_HIP(ctx, hipGetLastError());
    }
    RK_HIP(ctx, span.end());
    res->head.assign(head_bytes, 0);
    RK_HIP(ctx, hipMemcpyAsync(res->head.data(), head.p, head_bytes, hipMemcpyDeviceToHost, stream));
    RK_HIP(ctx, hipStreamSynchronize(stream));
    span.read();
    const uint64_t *off = (const uint64_t *)res->head.data();
    const uint64_t n_rec = off[Q];
    if (off[0] != 0 || n_rec > n_part) return rk_fail(ctx, RK_ERR_HIP, "rk_lca_rows: more records than partial records (internal error)");
    for (uint32_t q = 0; q < Q; q++)
        if (off[q + 1] < off[q]) return rk_fail(ctx, RK_ERR_HIP, "rk_lca_rows: offsets that do not ascend (internal error)");
    res->recs.resize(n_rec);
    if (n_rec) {
        RK_HIP(ctx, hipMemcpyAsync(res->recs.data(), rec.p, n_rec * sizeof(rk_lca_count), hipMemcpyDeviceToHost, stream));
        RK_HIP(ctx, hipStreamSynchronize(stream));
    }
    st->lists = U;
    st->postings = H;
    st->wave_lists = home.n_wave;
    st->block_lists = home.n_block;
    st->lane_lists = U - home.n_wave - home.n_block;
    st->partials = n_part;
    st->records = n_rec;
    st->longest_climb = home.longest;
    return RK_OK;
}

}  // namespace

extern "C" {

int rk_lca_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, const uint64_t *q_off, const uint64_t *q_lists, uint32_t n_query,
                 uint32_t n_ref, const uint32_t *taxa, const uint32_t *parent, uint32_t n_taxa, const rk_lca_opts *opts, uint64_t *off_out,
                 rk_lca_count **counts_out, uint64_t *n_counts, uint32_t *matched_out, uint32_t *unlabelled_out, rk_lca_stats *stats)
{
    if (!q_off || !opts || !off_out || !counts_out || !n_counts || !parent) return RK_ERR_ARG;
    if (n_query && (!matched_out || !unlabelled_out)) return RK_ERR_ARG;
    if (n_lists && !counts) return RK_ERR_ARG;
    if (n_ref >= 0x80000000u) return RK_ERR_UNSUPPORTED;
    std::vector<uint32_t> depth;
    uint32_t root = 0;
    if (int rc = check_taxonomy(parent, n_taxa, &depth, &root)) return rc;
    if (int rc = check_taxa(taxa, n_ref, n_taxa)) return rc;
    if (q_off[0] != 0) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++) {
        if (q_off[q + 1] < q_off[q]) return RK_ERR_ARG;
        if (q_off[q + 1] - q_off[q] > 0xFFFFFFFFULL) return RK_ERR_UNSUPPORTED;
    }
    if (q_off[n_query] && !q_lists) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        for (uint64_t j = q_off[q]; j < q_off[q + 1]; j++)
            if (q_lists[j] >= n_lists || (j > q_off[q] && q_lists[j - 1] > q_lists[j])) return RK_ERR_ARG;
    uint64_t total = 0;
    for (uint64_t u = 0; u < n_lists; u++) total += counts[u];
    if (total && !postings) return RK_ERR_ARG;
    for (uint64_t k = 0; k < total; k++)
        if (postings[k] >= n_ref) return RK_ERR_ARG;
    rk_lca_stats st;
    memset(&st, 0, sizeof st);
    fill_constants(&st, 0);
    st.path = 2;
    st.attempts = 1;
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, n_query);
    st.rows = (uint32_t)sel.rows.size();
    for (const uint32_t q : sel.rows) st.elements += q_off[q + 1] - q_off[q];
    HostResult r;
    lca_core(postings, counts, n_lists, q_off, q_lists, n_query, taxa, parent, depth.data(), sel, &r, &st);
    if (int rc = hand_out(view(r), sel, n_query, off_out, counts_out, n_counts, {matched_out, unlabelled_out})) return rc;
    if (stats) *stats = st;
    return RK_OK;
}

int rk_lca_call(const rk_lca_count *counts, const uint64_t *off, uint32_t n_query, const uint32_t *query_sizes, const uint32_t *parent, uint32_t n_taxa,
                const rk_lca_rule *rule, rk_lca_called *called_out, uint32_t *clade_out)
{
    if (!off || !parent || !rule || (n_query && !called_out)) return RK_ERR_ARG;
    if (!rule->min_count || !rule->conf_den || rule->conf_num > rule->conf_den || rule->denom > 1) return RK_ERR_ARG;
    if (rule->denom == 1 && n_query && !query_sizes) return RK_ERR_ARG;
    std::vector<uint32_t> depth;
    uint32_t root = 0;
    if (int rc = check_taxonomy(parent, n_taxa, &depth, &root)) return rc;
    if (off[0] != 0) return RK_ERR_ARG;
    for (uint32_t q = 0; q < n_query; q++)
        if (off[q + 1] < off[q]) return RK_ERR_ARG;
    if (off[n_query] && !counts) return RK_ERR_ARG;
    std::vector<unsigned char> seen(n_taxa, 0);
    for (uint32_t q = 0; q < n_query; q++) {
        bool bad = false;
        uint64_t sum = 0;   // the fields of rk_lca_called are 32 bits wide: a tally of rk_lca_rows fits, one of the caller's may not
        for (uint64_t j = off[q]; j < off[q + 1]; j++) {
            if (counts[j].taxon >= n_taxa || seen[counts[j].taxon]) bad = true;
            else seen[counts[j].taxon] = 1;
            sum += counts[j].direct;
        }
        for (uint64_t j = off[q]; j < off[q + 1]; j++)
            if (counts[j].taxon < n_taxa) seen[counts[j].taxon] = 0;
        if (bad) return RK_ERR_ARG;
        if (sum > 0xFFFFFFFFULL) return RK_ERR_UNSUPPORTED;
    }
    // direct[t] / clade[t] of the query at hand, cleared through `touched` after it: a query costs its records times their depth
    std::vector<uint64_t> direct(n_taxa, 0), clade(n_taxa, 0);
    std::vector<uint32_t> touched;
    std::vector<rk_lca_called> called(n_query);
    std::vector<uint32_t> clades(clade_out ? off[n_query] : 0);
    for (uint32_t q = 0; q < n_query; q++) {
        rk_lca_called c = {kNone, kNone, 0, 0, 0, 0};
        uint64_t retained = 0;
        touched.clear();
        for (uint64_t j = off[q]; j < off[q + 1]; j++)
            if (counts[j].direct >= rule->min_count) {
                const uint32_t t = counts[j].taxon;
                direct[t] = counts[j].direct;
                retained += counts[j].direct;
                c.n_taxa++;
                for (uint32_t at = t;; at = parent[at]) {
                    if (!clade[at]) touched.push_back(at);
                    clade[at] += counts[j].direct;
                    if (at == root) break;
                }
            }
        c.retained = (uint32_t)retained;
        if (c.n_taxa) {
            uint64_t best = 0;
            uint32_t cand = kNone;
            for (uint64_t j = off[q]; j < off[q + 1]; j++)
                if (counts[j].direct >= rule->min_count) {
                    const uint32_t t = counts[j].taxon;
                    uint64_t score = 0;
                    for (uint32_t at = t;; at = parent[at]) {
                        score += direct[at];
                        if (at == root) break;
                    }
                    if (score > best) {
                        best = score;
                        cand = t;
                    } else if (score == best) {
                        cand = lca2(parent, depth.data(), cand, t);
                    }
                }
            c.candidate = cand;
            c.score = (uint32_t)best;
            const uint64_t D = rule->denom ? query_sizes[q] : retained;
            c.clade = (uint32_t)clade[root];
            for (uint32_t at = cand;; at = parent[at]) {
                if (clade[at] * rule->conf_den >= (uint64_t)rule->conf_num * D) {
                    c.taxon = at;
                    c.clade = (uint32_t)clade[at];
                    break;
                }
                if (at == root) break;
            }
        }
        if (clade_out)
            for (uint64_t j = off[q]; j < off[q + 1]; j++) clades[j] = (uint32_t)clade[counts[j].taxon];
        for (const uint32_t t : touched) clade[t] = 0;
        for (uint64_t j = off[q]; j < off[q + 1]; j++) direct[counts[j].taxon] = 0;
        called[q] = c;
    }
    if (n_query) memcpy(called_out, called.data(), (size_t)n_query * sizeof(rk_lca_called));
    if (clade_out && !clades.empty()) memcpy(clade_out, clades.data(), clades.size() * 4);
    return RK_OK;
}

int rk_lca_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const uint32_t *taxa, const uint32_t *parent, uint32_t n_taxa,
                const rk_lca_opts *opts, uint64_t *off_out, rk_lca_count **counts_out, uint64_t *n_counts, uint32_t *matched_out, uint32_t *unlabelled_out,
                rk_lca_stats *stats)
{
    if (!ctx || !idx || !queries || !parent || !opts || !off_out || !counts_out || !n_counts) return RK_ERR_ARG;
    const char *const who = "rk_lca_rows";
    const uint32_t N = idx->n_ref, Q = queries->n;
    if (Q && (!matched_out || !unlabelled_out)) return rk_fail(ctx, RK_ERR_ARG, "%s: matched_out or unlabelled_out is null", who);
    if (N && !taxa) return rk_fail(ctx, RK_ERR_ARG, "%s: taxa is null", who);
    if (!n_taxa) return rk_fail(ctx, RK_ERR_ARG, "%s: a taxonomy without nodes", who);
    if (n_taxa >= 0x80000000u || N >= 0x80000000u) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: 2^31 nodes or references and more", who);
    std::vector<uint32_t> depth;
    uint32_t root = 0;
    if (check_taxonomy(parent, n_taxa, &depth, &root))
        return rk_fail(ctx, RK_ERR_ARG, "%s: the taxonomy needs exactly one root (parent[t] == t), parents below n_taxa and no cycle", who);
    if (check_taxa(taxa, N, n_taxa)) return rk_fail(ctx, RK_ERR_ARG, "%s: a taxon that is neither a node nor RK_LCA_NONE", who);
    if (queries->wide != idx->wide) return rk_fail(ctx, RK_ERR_ARG, "query sketches and index use different hash widths");
    if (N && (!idx->d_postings || !idx->d_upos || idx->n_shards > 1))
        return rk_fail(ctx, RK_ERR_ARG, "%s: an index without all posting lists (rk_index_join_shard, one hash range of a sharded build)", who);
    if (queries->max_size > 0xFFFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: a query sketch of 2^32 elements or more", who);
    rk_lca_stats st;
    memset(&st, 0, sizeof st);
    const TimedSpan span{ctx, RK_MS_LCA};
    span.clear();
    const RowSel sel(opts->row_first, opts->row_step, opts->row_block, Q);
    st.rows = (uint32_t)sel.rows.size();
    for (const uint32_t q : sel.rows) st.elements += queries->h_off[q + 1] - queries->h_off[q];
    uint32_t *const outs[2] = {matched_out, unlabelled_out};
    HostResult host;
    DeviceResult dev;
    Result r;
    const bool runs = N && idx->U && !sel.rows.empty();   // (else no element has a posting list: r stays without offsets)
    if (runs) fill_constants(&st, queries->total);
    if (runs && rk_switched_off("RK_LCA_DEVICE")) {
        st.path = 2;
        st.attempts = 1;
        RK_TRY(idx->wide ? lca_on_host<uint64_t>(ctx, idx, queries, taxa, parent, depth.data(), sel, &host, &st)
                         : lca_on_host<uint32_t>(ctx, idx, queries, taxa, parent, depth.data(), sel, &host, &st));
        r = view(host);
    } else if (runs) {
        st.path = 1;
        RK_TRY(lca_on_device(ctx, idx, queries, taxa, parent, n_taxa, root, opts, &st, &dev));
        r = Result::from_block(dev.head.data(), Q, dev.recs.size());
        r.recs = dev.recs.data();   // (the records come home in a copy of their own)
        for (const uint32_t q : sel.rows) {
            st.matched += r.per_row[0][q];
            st.unlabelled += r.per_row[1][q];
        }
    }
    if (hand_out(r, sel, Q, off_out, counts_out, n_counts, outs)) return rk_fail(ctx, RK_ERR_NOMEM, "%s: out of host memory", who);
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
