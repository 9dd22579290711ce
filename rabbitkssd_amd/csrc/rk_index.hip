// rk_index.hip -- device-side inverted index (replaces transSketches, src/sketch.cpp:970-1017,
// and the .index load + prefix sum of src/dist.cpp:86-129).
//
// HBM layout of an index over N genomes, H postings, U distinct hashes:
//   postings  u32[H]    genome ids ordered (hash asc, genome asc)      == the .dict payload
//   uhash     u32[U]    sorted distinct hashes                         (compact, not 2^bits)
//   upos      u32[U+1]  posting offsets of each distinct hash
//   sizes     u32[N]    sketch sizes
//   selfrange uint2[n_self]  for every source element (genome g, hash h) with later sharers: the slice of h's posting
//                       list holding genomes > g (the all-vs-all triangle needs no lookup), either as the posting range
//                       (x, y) or, when the genomes lie within 32 ids, COMPACT as (bit 31 | first genome, bitmask of
//                       the ids first .. first+31); rows back to back, inside a row the slices "covered" by the
//                       pair partner last (self_split)
// Derived on demand and cached: dir (prefix directory into uhash, for 64-bit / > 2^30 hash spaces), the rank bitmap
// of the query path (rk_distq.hip), sum of squared list lengths.  The dense 2^bits count array of the .index file
// is only materialised by rk_index_export / consumed by rk_index_import.
//
// This unit holds the build (plan, stages, renumbering), the products built on first use (slice records, prefix directory),
// the accessors, rk_index_free and the sharded build with its exchange.  What moves a finished index in or out -- imports,
// exports, the single-buffer blob, rk_index_broadcast -- is rk_index_io.hip.
//
// Build = ONE library primitive (rocprim radix sort of (hash, source element)) + 7 small kernels on the context's
// stream, every buffer from the context's pool, ONE 32-byte read-back at the end: no hipMalloc, no hipFree and
// no intermediate synchronisation in steady state.
#include <cstring>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <thread>

#include "rk_internal.h"

namespace {

struct BuildResult {  // written by the kernels, read back once
    unsigned long long U, n_self, dups, flags;
    unsigned long long flagged;   // slice records that are near-flagged posting ranges (fast path only): related lists wider than a compact record
};

// Single-workgroup exclusive scan: store(i, sum of load(j), j < i) for i < n; returns the grand total.  The array is taken as
// rows of 64 (lane = column: every load and store of a wave is one coalesced access -- round 4; a thread owning a contiguous
// stretch made each access 64 separate lines), a wave owns R consecutive rows of every stretch of nw * R rows and holds them
// in registers: all its loads are in flight at once, so a stretch (16,384 entries with 16 waves) costs ONE memory round trip,
// a block-wide exchange of the waves' totals and R wave scans with a running carry.
template <class Acc, class L, class W> __device__ inline Acc block_scan_sweeps(uint32_t n, L load, W store)
{
    __shared__ Acc scan_part[1024 / 64];
    constexpr uint32_t R = 16;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const uint32_t rows = (n + 63) / 64;
    Acc carry = 0;
    for (uint32_t base = 0; base < rows; base += nw * R) {
        const uint32_t r0 = base + wave * R;
        Acc v[R], sum = 0;
#pragma unroll
        for (uint32_t u = 0; u < R; u++) {
            const uint32_t i = (r0 + u) * 64 + lane;
            v[u] = i < n ? load(i) : Acc(0);
        }
#pragma unroll
        for (uint32_t u = 0; u < R; u++) sum += v[u];
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) scan_part[wave] = sum;
        __syncthreads();
        Acc run = carry, all = 0;
        for (uint32_t w = 0; w < nw; w++) {
            if (w < wave) run += scan_part[w];
            all += scan_part[w];
        }
#pragma unroll
        for (uint32_t u = 0; u < R; u++) {
            const uint32_t i = (r0 + u) * 64 + lane;
            if ((r0 + u) * 64 < n) {   // (wave-uniform)
                Acc incl = v[u];
                for (int o = 1; o < 64; o <<= 1) {
                    const Acc t = __shfl_up(incl, o);
                    if ((int)lane >= o) incl += t;
                }
                if (i < n) store(i, run + incl - v[u]);
                run += __shfl(incl, 63);
            }
        }
        carry += all;
        __syncthreads();
    }
    return carry;
}

__global__ void k_sizes(const uint64_t *off, uint32_t n, uint32_t *sizes, uint64_t *off_copy)
{
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) sizes[g] = (uint32_t)(off[g + 1] - off[g]);
    if (g <= n) off_copy[g] = off[g];
}

// one wave per genome: gid[e] = genome of source element e, iota[e] = e (the sort's value array)
__global__ void k_fill_gid(const uint64_t *off, uint32_t n_genomes, uint32_t *gid, uint32_t *iota)
{
    const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint64_t e1 = off[g + 1];
    for (uint64_t e = off[g] + (threadIdx.x & 63); e < e1; e += 64) {
        gid[e] = g;
        iota[e] = (uint32_t)e;
    }
}

template <class K> __global__ void k_head_flags(const K *keys, uint64_t n, uint32_t *flags)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) flags[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1u : 0u;
}

// gidx = inclusive scan of head flags (1-based group number)
template <class K>
__global__ void k_scatter_heads(const K *keys, const uint32_t *gidx, uint64_t n, K *uhash, uint32_t *upos, BuildResult *res)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t g = gidx[k] - 1;
    if (k == 0 || gidx[k - 1] != gidx[k]) {
        uhash[g] = keys[k];
        upos[g] = (uint32_t)k;
    }
    if (k == n - 1) {
        upos[g + 1] = (uint32_t)n;
        res->U = (unsigned long long)g + 1;
    }
}

// class of a source element's "later genomes" slice, carried by the slice itself so that no separate (byte-granular,
// randomly scattered) class array is needed: (x, y) with x < y = open, x == y = empty, stored reversed (y, x) = covered
enum : uint8_t { kEmpty = 0, kOpen = 1, kCovered = 2 };
__device__ inline uint8_t slice_class(uint2 r) { return r.x == r.y ? kEmpty : (r.x < r.y ? kOpen : kCovered); }
__device__ inline uint2 slice_range(uint2 r) { return r.x <= r.y ? r : make_uint2(r.y, r.x); }

// postings[k] = genome of the k-th sorted element; selfrange of its source element = (k+1, end of the group): the
// sort is stable and source elements are genome-major, so the rest of the group holds the later genomes.
// covered (self join, row pairs): genome 2p+1 shares this hash with genome 2p, i.e. its predecessor in the posting
// list is its pair partner.  Walking the partner's slice then serves both rows (the slice of 2p starts with 2p+1 and
// continues with exactly the slice of 2p+1), so the pair kernel skips the covered slices of the odd row.
// CHECK_DUPS (sketches not known to be sets): a genome that repeats a hash sits next to itself in the group.
template <bool CHECK_DUPS, bool NO_SELF = false>
__global__ void k_postings_selfrange(const uint32_t *sorted_e, const uint32_t *gidx, const uint32_t *upos,
                                     const uint32_t *gid, uint64_t n, uint32_t *postings, uint2 *self_raw,
                                     BuildResult *res)
{
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t e = sorted_e[k];
    const uint32_t me = gid[e];
    postings[k] = me;
    if (NO_SELF) return;   // (an index without slice records: set sketches, nothing to check)
    const uint32_t g = gidx[k] - 1;
    const uint32_t end = upos[g + 1];
    const bool has_prev = k > upos[g];
    uint32_t prev = 0xFFFFFFFFu;
    if (has_prev && (CHECK_DUPS || (me & 1u))) prev = gid[sorted_e[k - 1]];
    if (CHECK_DUPS && has_prev && prev == me) res->dups = 1;
    const bool covered = (me & 1u) && has_prev && prev == me - 1 && (uint32_t)k + 1 < end;
    self_raw[e] = covered ? make_uint2(end, (uint32_t)k + 1) : make_uint2((uint32_t)k + 1, end);
}

// one wave per genome: number of open / covered slices of its row
__global__ void k_row_counts(const uint64_t *off, uint32_t n_genomes, const uint2 *self_raw, uint32_t *n_open, uint32_t *n_cov)
{
    const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t e1 = off[g + 1];
    uint32_t no = 0, nc = 0;
    for (uint64_t e = off[g] + lane; e < e1; e += 64) {
        const uint8_t c = slice_class(self_raw[e]);
        no += c == kOpen;
        nc += c == kCovered;
    }
    for (int o = 32; o > 0; o >>= 1) {
        no += __shfl_down(no, o);
        nc += __shfl_down(nc, o);
    }
    if (lane == 0) {
        n_open[g] = no;
        n_cov[g] = nc;
    }
}

// single workgroup: self_off = exclusive scan of the row lengths, self_split = where a row's covered slices start
__global__ void k_row_scan(const uint32_t *n_open, const uint32_t *n_cov, uint32_t n_genomes, uint64_t *self_off,
                           uint64_t *self_split, BuildResult *res)
{
    const unsigned long long all = block_scan_sweeps<unsigned long long>(
        n_genomes, [&](uint32_t g) { return (unsigned long long)n_open[g] + n_cov[g]; },
        [&](uint32_t g, unsigned long long before) {
            self_off[g] = before;
            self_split[g] = before + n_open[g];
        });
    if (threadIdx.x == 0) {
        self_off[n_genomes] = all;
        self_split[n_genomes] = all;
        res->n_self = all;
    }
}

// A slice whose genomes all lie within 32 ids -- the normal case in a collection ordered by similarity, where a hash is
// shared by a handful of neighbouring strains -- is stored COMPACT: (bit 31 | first genome, bitmask of the genomes
// first+0 .. first+31; bit 0 is always set).  The distance kernel then needs no posting load for it at all: the
// 8-byte slice record IS the posting list.  Other slices stay posting ranges (x, y), x < 2^31.
// A slice that stays a posting range carries the NEAR flag in bit 31 of y: its first genome lies within 32 ids of the
// element's own genome g (only then can it have members inside the window of rk_near_kernel).
__device__ inline uint2 compact_slice(uint2 r, const uint32_t *postings, uint32_t g, bool compact)
{
    const uint32_t first = postings[r.x], last = postings[r.y - 1];
    if (!compact || last - first > 31u) return make_uint2(r.x, r.y | (first - g <= 32u ? 0x80000000u : 0u));
    uint32_t mask = 1;
    for (uint32_t k = r.x + 1; k < r.y; k++) mask |= 1u << (postings[k] - first);
    return make_uint2(0x80000000u | first, mask);
}

// one wave per genome: open slices to the front of the row, covered ones behind them, empty ones dropped; the order
// inside each class is the source order (ballot ranks)
// compact: the sketches are sets.  A genome that repeats a hash sits several times in the list and must be counted as
// often (src/dist.cpp:199-202): a bitmask cannot say that, so the slices of a multiset index stay posting ranges.
__global__ void k_row_place(const uint64_t *off, uint32_t n_genomes, const uint2 *self_raw,
                            const uint64_t *self_off, const uint64_t *self_split, const uint32_t *postings, bool compact, uint2 *out)
{
    const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long lt = lane ? (~0ULL >> (64 - lane)) : 0ULL;
    uint64_t at_open = self_off[g], at_cov = self_split[g];
    const uint64_t e0 = off[g], e1 = off[g + 1];
    for (uint64_t base = e0; base < e1; base += 64) {
        const uint64_t e = base + lane;
        const uint2 raw = e < e1 ? self_raw[e] : make_uint2(0, 0);
        const uint8_t c = slice_class(raw);
        uint2 r = slice_range(raw);
        if (c != kEmpty) r = compact_slice(r, postings, g, compact);
        const unsigned long long mo = __ballot(c == kOpen), mc = __ballot(c == kCovered);
        if (c == kOpen) out[at_open + __popcll(mo & lt)] = r;
        if (c == kCovered) out[at_cov + __popcll(mc & lt)] = r;
        at_open += __popcll(mo);
        at_cov += __popcll(mc);
    }
}

template <class K>
__global__ void k_dir(const K *uhash, uint64_t U, int shift, uint32_t n_buckets, uint32_t *dir)
{
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_buckets) return;
    if (b == n_buckets) { dir[b] = (uint32_t)U; return; }
    const uint64_t key = (uint64_t)b << shift;
    uint64_t lo = 0, hi = U;  // first index with uhash >= key
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)uhash[mid] < key) lo = mid + 1; else hi = mid;
    }
    dir[b] = (uint32_t)lo;
}

__global__ void k_sum_sq(const uint32_t *upos, uint64_t U, unsigned long long *acc)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = 0;
    if (i < U) {
        unsigned long long c = upos[i + 1] - upos[i];
        v = c * c;
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __shared__ unsigned long long part[kThreads / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kThreads / 64; w++) t += part[w];
        if (t) atomicAdd(acc, t);
    }
}

// one wave per genome: compact records of its row, records the pair kernel walks (all of an even row, the uncovered of an odd one)
__global__ void k_self_stats(const uint2 *selfrange, const uint64_t *self_off, const uint64_t *self_split, uint32_t n_genomes,
                             unsigned long long *acc)
{
    const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t e0 = self_off[g], e1 = self_off[g + 1];
    unsigned long long cpt = 0;
    for (uint64_t e = e0 + lane; e < e1; e += 64) cpt += selfrange[e].x >> 31;
    for (int o = 32; o > 0; o >>= 1) cpt += __shfl_down(cpt, o);
    if (lane == 0) {
        if (cpt) atomicAdd(&acc[0], cpt);
        atomicAdd(&acc[1], (unsigned long long)(((g & 1u) ? self_split[g] : e1) - e0));
    }
}

// ---- internal genome order ------------------------------------------------------------------------------------
// Compact slices, list records and row pairs pay off when the genomes that share a hash have neighbouring ids.  A
// collection arrives in whatever order its files were listed (or completed, src/sketch.cpp:558-568), so the build
// renumbers it: genomes are clustered by their kMinK smallest hashes (a bottom-k MinHash of the sketch: two genomes
// with Jaccard similarity j share each of them with probability ~j), every genome attaches to the smallest-id genome
// that shares at least two of them, clusters become runs of consecutive internal ids (ordered by their smallest
// member, members by their original id -- a collection that already lists relatives together keeps its order).
// The clustering only shapes the data layout: every count stays exact whatever it decides.
constexpr uint32_t kMinK = 16;
constexpr unsigned long long kEmptySlot = ~0ULL;
__device__ inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
template <class K> __device__ inline uint32_t fold_hash(K h)
{
    if constexpr (sizeof(K) == 8) return (uint32_t)(h ^ (h >> 32));
    else return (uint32_t)h;
}

// What the renumbering reads of genome g: the count and the values of its first min(size, kMinK) hashes, folded to 32 bits -- from the
// sketches' CSR, or from the all-gathered signatures of a build from keys (rk_index_keys.inc: size, then those hashes, folded already)
template <class K> struct CsrMinK {
    const K *hashes;
    const uint64_t *off;
    __device__ uint32_t count(uint32_t g) const { return (uint32_t)min((uint64_t)kMinK, off[g + 1] - off[g]); }
    __device__ uint32_t at(uint32_t g, uint32_t i) const { return fold_hash(hashes[off[g] + i]); }
};
struct SigMinK {
    const uint32_t *sig;   // RK_SIG_WORDS u32 per genome
    __device__ uint32_t count(uint32_t g) const { return min(kMinK, sig[(size_t)g * RK_SIG_WORDS]); }
    __device__ uint32_t at(uint32_t g, uint32_t i) const { return sig[(size_t)g * RK_SIG_WORDS + 1 + i]; }
};

// table slot = (hash << 32 | smallest genome that lists the hash among its kMinK smallest); open addressing.
// (round 5) A workgroup holds 64 neighbouring genomes -- relatives, in a collection listed species by species -- and first settles
// "the smallest genome per hash" among ITS 1,024 elements in an LDS table; only the winners go to the device-wide table.  Its loads
// and atomics are device-scope round trips (~30 us per million, and whatever streams beside them waits: 0.55 ms at 500,000 genomes,
// paid by every shard of a sharded build); among relatives an LDS table leaves a sixteenth of them.
constexpr uint32_t kInsertThreads = 1024, kInsertLocal = 2048;
__device__ inline void minhash_insert_global(unsigned long long *table, uint32_t mask, unsigned long long mine)
{
    const uint32_t h = (uint32_t)(mine >> 32);
    uint32_t slot = mix32(h) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        unsigned long long cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmptySlot) {
            cur = atomicCAS(&table[slot], kEmptySlot, mine);
            if (cur == kEmptySlot) return;
        }
        if ((uint32_t)(cur >> 32) == h) {
            // (the slot only ever decreases: a genome that finds a smaller one there has nothing to add)
            if (cur > mine) atomicMin(&table[slot], mine);
            return;
        }
        slot = (slot + 1) & mask;
    }
}
template <class Src>
__global__ __launch_bounds__(kInsertThreads) void k_minhash_insert(Src src, uint32_t n_genomes, unsigned long long *table, uint32_t mask)
{
    __shared__ unsigned long long loc[kInsertLocal];   // (at most half full: 1,024 elements)
    for (uint32_t s = threadIdx.x; s < kInsertLocal; s += kInsertThreads) loc[s] = kEmptySlot;
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * kInsertThreads + threadIdx.x;
    const uint32_t g = (uint32_t)(t / kMinK), i = (uint32_t)(t % kMinK);
    if (g < n_genomes) {
        if (i < src.count(g)) {
            const uint32_t h = src.at(g, i);
            const unsigned long long mine = ((unsigned long long)h << 32) | g;
            uint32_t slot = (mix32(h) >> 11) & (kInsertLocal - 1);   // (other bits than the device-wide table's)
            for (uint32_t probe = 0; probe < kInsertLocal; probe++) {
                unsigned long long cur = loc[slot];
                if (cur == kEmptySlot) {
                    cur = atomicCAS(&loc[slot], kEmptySlot, mine);
                    if (cur == kEmptySlot) break;
                }
                if ((uint32_t)(cur >> 32) == h) {
                    if (cur > mine) atomicMin(&loc[slot], mine);
                    break;
                }
                slot = (slot + 1) & (kInsertLocal - 1);
            }
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < kInsertLocal; s += kInsertThreads) {
        const unsigned long long v = loc[s];
        if (v != kEmptySlot) minhash_insert_global(table, mask, v);
    }
}

// parent[g] = the smallest genome below g that shares at least two of g's kMinK smallest hashes (g itself if none)
template <class Src>
__global__ void k_minhash_vote(Src src, uint32_t n_genomes, const unsigned long long *table, uint32_t mask, uint32_t *parent)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genomes) return;
    const uint32_t n = src.count(g);
    uint32_t r[kMinK];
#pragma unroll
    for (uint32_t i = 0; i < kMinK; i++) {
        r[i] = g;
        if (i < n) {
            const uint32_t h = src.at(g, i);
            uint32_t slot = mix32(h) & mask;
            for (uint32_t probe = 0; probe <= mask; probe++) {
                const unsigned long long cur = table[slot];
                if (cur == kEmptySlot) break;
                if ((uint32_t)(cur >> 32) == h) { r[i] = (uint32_t)cur; break; }
                slot = (slot + 1) & mask;
            }
        }
    }
    uint32_t best = g;
#pragma unroll
    for (uint32_t i = 0; i < kMinK; i++) {
        uint32_t votes = 0;
#pragma unroll
        for (uint32_t j = 0; j < kMinK; j++) votes += r[j] == r[i];
        if (votes >= 2 && r[i] < best) best = r[i];
    }
    parent[g] = best;
}

// key[g] = (root of g's cluster, g): parents only ever point to smaller ids, so the walk ends at a fixed point
__global__ void k_cluster_keys(const uint32_t *parent, uint32_t n_genomes, int id_bits, unsigned long long *keys)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genomes) return;
    uint32_t p = parent[g];
    for (uint32_t hop = 0; hop < n_genomes; hop++) {
        const uint32_t q = parent[p];
        if (q == p) break;
        p = q;
    }
    keys[g] = ((unsigned long long)p << id_bits) | g;
}

// sorted keys -> orig[internal id], sizes in internal order
// (sizes_in: the sizes in the caller's order, when there is no CSR -- a build from keys)
__global__ void k_order_from_keys(const unsigned long long *keys, uint32_t n_genomes, int id_bits, const uint64_t *off,
                                  const uint32_t *sizes_in, uint32_t *orig, uint32_t *sizes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_genomes) return;
    const uint32_t g = (uint32_t)(keys[i] & ((1ULL << id_bits) - 1ULL));
    orig[i] = g;
    sizes[i] = sizes_in ? sizes_in[g] : (uint32_t)(off[g + 1] - off[g]);
}

// single workgroup: off_new = exclusive scan of the sizes in internal order
__global__ void k_offsets_scan(const uint32_t *sizes, uint32_t n_genomes, uint64_t *off_new)
{
    const unsigned long long all = block_scan_sweeps<unsigned long long>(
        n_genomes, [&](uint32_t g) { return (unsigned long long)sizes[g]; },
        [&](uint32_t g, unsigned long long before) { off_new[g] = before; });
    if (threadIdx.x == 0) off_new[n_genomes] = all;
}

// Small collections (<= 32,768 genomes): the (root, genome) keys are ordered by COUNTING -- the keys are distinct, so a
// key's position is the number of smaller keys; every workgroup compares 256 keys with a stretch of 512 others (scalar
// loads: the stretch is the same for all lanes) and adds its partial counts.  10,000 keys: 800 workgroups, a few
// microseconds -- a device-wide sort of so few keys costs 70 us of launches.
constexpr uint32_t kRankThreads = 256, kRankPer = 4, kRankQ = kRankThreads * kRankPer, kRankStretch = 256, kRankMaxN = 32768;
// (root, genome) packed into 32 bits: 2 * id_bits <= 30 for up to 32,768 genomes
// (also zeroes the rank counters k_rank_keys adds to: a fill of its own is one more 6 us dispatch in the chain)
__global__ void k_cluster_keys32(const uint32_t *parent, uint32_t n_genomes, int id_bits, uint32_t *keys, uint32_t *rank)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genomes) return;
    rank[g] = 0;
    uint32_t p = parent[g];
    for (uint32_t hop = 0; hop < n_genomes; hop++) {
        const uint32_t q = parent[p];
        if (q == p) break;
        p = q;
    }
    keys[g] = (p << id_bits) | g;
}
// every thread ranks kRankPer keys against a stretch of 256 others staged in LDS (16-byte broadcast reads: four
// others per read, sixteen comparisons per read)
__global__ __launch_bounds__(kRankThreads) void k_rank_keys(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *rank)
{
    __shared__ __attribute__((aligned(16))) uint32_t others[kRankStretch];
    const uint32_t j0 = blockIdx.y * kRankStretch;
    for (uint32_t j = threadIdx.x; j < kRankStretch; j += kRankThreads) others[j] = j0 + j < n ? keys[j0 + j] : 0xFFFFFFFFu;
    uint32_t mine[kRankPer], below[kRankPer];
#pragma unroll
    for (uint32_t i = 0; i < kRankPer; i++) {
        const uint32_t q = blockIdx.x * kRankQ + i * kRankThreads + threadIdx.x;
        mine[i] = q < n ? keys[q] : 0u;
        below[i] = 0;
    }
    __syncthreads();
    const uint4 *o4 = reinterpret_cast<const uint4 *>(others);
#pragma unroll 4
    for (uint32_t j = 0; j < kRankStretch / 4; j++) {
        const uint4 v = o4[j];
#pragma unroll
        for (uint32_t i = 0; i < kRankPer; i++) below[i] += (v.x < mine[i]) + (v.y < mine[i]) + (v.z < mine[i]) + (v.w < mine[i]);
    }
#pragma unroll
    for (uint32_t i = 0; i < kRankPer; i++) {
        const uint32_t q = blockIdx.x * kRankQ + i * kRankThreads + threadIdx.x;
        if (q < n && below[i]) atomicAdd(&rank[q], below[i]);
    }
}
__global__ void k_order_from_rank(const uint32_t *rank, uint32_t n_genomes, const uint64_t *off, const uint32_t *sizes_in, uint32_t *orig, uint32_t *sizes)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genomes) return;
    const uint32_t i = rank[g];   // (the g-th key belongs to genome g: k_cluster_keys32)
    orig[i] = g;
    sizes[i] = sizes_in ? sizes_in[g] : (uint32_t)(off[g + 1] - off[g]);
}

// one wave per internal genome: its hashes move to their place in the internal-order CSR
template <class K>
__global__ void k_gather_sketches(const K *hashes, const uint64_t *off, const uint32_t *orig, const uint64_t *off_new,
                                  uint32_t n_genomes, K *out)
{
    const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n_genomes) return;
    const uint64_t src = off[orig[i]], dst = off_new[i], n = off_new[i + 1] - dst;
    for (uint64_t k = threadIdx.x & 63; k < n; k += 64) out[dst + k] = hashes[src + k];
}

// inv[orig[i]] = i
// tab[caller's genome] = (internal id, start of its sketch in the internal-order element space): what k_bucket_emit needs of
// a key's genome, in one gather (the fast build takes H < 2^30)
__global__ void k_emit_table(const uint32_t *inv, const uint64_t *off_new, uint32_t n, uint2 *tab)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) tab[g] = make_uint2(inv[g], (uint32_t)off_new[inv[g]]);
}

__global__ void k_invert_order(const uint32_t *orig, uint32_t n, uint32_t *inv)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) inv[orig[i]] = i;
}

__global__ void k_iota(uint32_t n, uint32_t *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

#include "rk_index_fast.inc"
#include "rk_index_tiles.inc"
#include "rk_index_keys.inc"

// What a build reads of its GENOMES (sizes and offsets, the hashes the renumbering looks at, whether they are sets) and of its
// ELEMENTS (the partition source): the sketches themselves (rk_index_build, rk_index_build_shard), or the keys of one shard that
// arrived from every rank with the all-gathered signatures of the genomes (rk_index_build_shard_keys).
struct BuildSource {
    uint32_t n = 0;                        // genomes
    uint64_t total = 0;                    // postings of the whole collection
    bool wide = false, is_set = false;
    uint64_t max_size = 0, min_size = 0;   // largest, smallest non-empty sketch
    const uint64_t *d_off = nullptr;       // u64[n + 1]: CSR offsets of the sketches (caller's order), or
    const uint32_t *d_sizes = nullptr;     // u32[n]: the sizes (caller's order) and
    const uint32_t *d_sig = nullptr;       // the signatures (RK_SIG_WORDS u32 per genome) the renumbering reads -- a build from keys
    const rk_sketches *s = nullptr;        // elements: the sketches, or
    const unsigned long long *keys = nullptr;   // the shard's keys (wire format of rk_sketches_shard_pack), n_keys of them
    uint64_t n_keys = 0;
};
inline BuildSource source_of(const rk_sketches *s)
{
    BuildSource src;
    src.n = s->n;
    src.total = s->total;
    src.wide = s->wide;
    src.is_set = s->is_set;
    src.max_size = s->max_size;
    for (uint32_t g = 0; g < s->n; g++) {
        const uint64_t sz = s->h_off[g + 1] - s->h_off[g];
        if (sz && (!src.min_size || sz < src.min_size)) src.min_size = sz;
    }
    src.d_off = s->d_off;
    src.s = s;
    return src;
}

// ==== the index build, host side: plan -> index arrays -> bucket-sort attempts -> general path -> finish ====
#include "rk_index_plan.h"

// The tile sort's buffers (launch_tile_sort): what the build and rk_index_join_shard both set up, sort into and hand to the index.
struct TileSortBufs {
    DevBuf<uint3> brec;                       // the records binned by row block
    DevBuf<uint32_t> tb, bins, t_rows, t_cols;
    DevBuf<uint4> proto, t_dir_j, t_dir_c;    // the directory's proto entries, the directories
    DevBuf<unsigned long long> level_start;
    DevBuf<uint2> t_contrib;
    explicit TileSortBufs(rk_ctx *c) : brec(c), tb(c), bins(c), t_rows(c), t_cols(c), proto(c), t_dir_j(c), t_dir_c(c), level_start(c), t_contrib(c) {}
    int alloc(rk_ctx *ctx, uint32_t n_blocks, uint64_t n_records, uint64_t tile_cap)
    {
        const uint64_t slot_cap = n_records + tile_cap;   // (every tile from an even slot on)
        RK_HIP(ctx, brec.alloc(n_records));
        RK_HIP(ctx, tb.alloc(3 * (size_t)n_blocks));
        RK_HIP(ctx, bins.alloc((size_t)n_blocks + 1));   // bin starts (the counts and cursors are in `zeroed`)
        RK_HIP(ctx, proto.alloc(2 * tile_cap));
        RK_HIP(ctx, level_start.alloc(2 * (kTileTable + 1)));
        RK_HIP(ctx, t_contrib.alloc(slot_cap + 256));
        if (rowsort_stage(n_blocks)) {   // (the split copy serves the scalar-row variant of the tile kernel: short launches over small collections)
            RK_HIP(ctx, t_rows.alloc(slot_cap + 256));
            RK_HIP(ctx, t_cols.alloc(slot_cap + 256));
        }
        RK_HIP(ctx, t_dir_j.alloc(2 * tile_cap));
        RK_HIP(ctx, t_dir_c.alloc(2 * tile_cap));
        return RK_OK;
    }
    TileSortArgs args(const uint3 *rec, uint32_t region_cap, uint32_t n_blocks, const uint32_t *blk_min, const ZeroedLayout &z) const
    {
        TileSortArgs ta;
        memset(&ta, 0, sizeof ta);
        ta.rec = rec;
        ta.cur = z.tile_cursors();
        ta.region_cap = region_cap;
        ta.n_blocks = n_blocks;
        ta.bin_count = z.bin_count();
        ta.bin_cursor = z.bin_cursor();
        ta.bin_start = bins.p;
        ta.brec = brec.p;
        ta.blk_min = blk_min;
        ta.contrib = t_contrib.p;
        ta.rows = t_rows.p;
        ta.cols = t_cols.p;
        ta.tb_base = tb.p;
        ta.tb_cnt = tb.p + n_blocks;
        ta.order = tb.p + 2 * (size_t)n_blocks;
        ta.proto = proto.p;
        ta.level_start = level_start.p;
        ta.dir[0] = t_dir_j.p;
        ta.dir[1] = t_dir_c.p;
        ta.tres = z.tile_res();
        return ta;
    }
    void hand_over(rk_index *idx, const TileResult &tr)   // a finished sort: its results and counters into the index
    {
        idx->d_tile_contrib = t_contrib.release();
        idx->d_tile_rows = t_rows.release();
        idx->d_tile_cols = t_cols.release();
        idx->d_tile_dir[0] = t_dir_j.release();
        idx->d_tile_dir[1] = t_dir_c.release();
        idx->n_tile_slots = tr.n_slots;
        idx->n_tiles = tr.n_tiles;
        idx->n_tile_records = tr.n_records;
        idx->tile_max_records = tr.max_records;
        for (int m = 0; m < 2; m++)
            for (int k = 0; k < kTileTable; k++) idx->tile_prefix[m][k] = tr.level_count[m][k];
        idx->tiles_ready = true;
        idx->tiles_from_build = true;
    }
};

// what every stage of one build works on
struct BuildCtx {
    rk_ctx *ctx;
    const BuildSource &src;
    const BuildPlan &p;
    const BuildKnobs &k;
    rk_index *idx;
    hipStream_t st;   // the context's stream
};

int alloc_index_arrays(rk_ctx *ctx, rk_index *idx, const BuildPlan &p)
{
    RK_TRY(pool_array(ctx, &idx->d_sizes, (size_t)p.N + 1));
    RK_TRY(pool_array(ctx, &idx->d_src_off, (size_t)p.N + 1));
    RK_TRY(pool_array(ctx, &idx->d_postings, p.H_el + 8));   // (padded: the kernels read up to eight postings from any list start)
    if (idx->wide) RK_TRY(pool_array(ctx, &idx->d_uhash64, p.Ucap + 1));
    else RK_TRY(pool_array(ctx, &idx->d_uhash, p.Ucap + 1));
    RK_TRY(pool_array(ctx, &idx->d_upos, p.Ucap + 2));
    RK_TRY(pool_array(ctx, &idx->d_orig, (size_t)p.N + 1));
    if (p.tiles_mode) RK_TRY(pool_array(ctx, &idx->d_blk_min, (size_t)p.n_blocks));
    return RK_OK;
}
// (not for an index whose build emits tile records: rk_index_ensure_slices, on first use)
int alloc_slices(rk_ctx *ctx, rk_index *idx, const BuildPlan &p)
{
    if (p.no_self || idx->d_selfrange) return RK_OK;
    RK_TRY(pool_array(ctx, &idx->d_selfrange, p.H + 1));
    RK_TRY(pool_array(ctx, &idx->d_self_off, (size_t)p.N + 1));
    RK_TRY(pool_array(ctx, &idx->d_self_split, (size_t)p.N + 1));
    return RK_OK;
}
void drop_blk_min(rk_ctx *ctx, rk_index *idx)   // (no tile records after all)
{
    rk_pool_free(ctx, idx->d_blk_min);
    idx->d_blk_min = nullptr;
}

// the second stream of the build and the events of its fork/join protocol: created with the first build that uses them
int ensure_stream2(rk_ctx *ctx, bool high_priority)
{
    if (ctx->stream2) return RK_OK;
    // (its kernels are small and many: at the highest priority they are not queued behind the partition's workgroups)
    int prio_lo = 0, prio_hi = 0;
    if (high_priority && hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess && prio_hi != prio_lo)
        RK_HIP(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_hi));
    else
        RK_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    RK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    RK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    RK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_inv, hipEventDisableTiming));
    return RK_OK;
}

// ---- internal genome order: relatives next to each other (see k_minhash_insert) ---------------------------------
// d_orig, d_sizes and d_src_off (the CSR offsets in internal order); the rest of the build, and every kernel that
// uses the index, works in that order
// (round 4) It runs on a stream of its own: the partition of the hashes does not need it -- it walks the sketches
// in the CALLER's order and k_bucket_emit translates the genome ids through `inv` --, so the two overlap (≈ 70 us of
// small dependent kernels next to ≈ 160 us of partition); join() makes ctx->stream wait for it where its results are
// first used.  The temporaries live until the build returns (the pool's reuse is ordered on ctx->stream only): one
// Renumbering per build, destroyed with it.
struct Renumbering {
    const BuildCtx &b;
    DevBuf<unsigned long long> rl_table, rl_keys, rl_keys_sorted;
    DevBuf<uint32_t> rl_parent, rl_keys32, rl_rank, rl_inv;
    DevBuf<uint2> rl_tab;
    DevBuf<char> rl_tmp;   // the sort's scratch (kept until the build returns: the sort runs on the second stream)
    const uint32_t *inv = nullptr;   // caller's genome index -> internal id (null: identity)
    bool forked = false, joined = true;
    bool inv_recorded = false;   // ctx->ev_inv was recorded behind the kernel that completes `inv`
    bool enqueued = false;
    explicit Renumbering(const BuildCtx &bc)
        : b(bc), rl_table(bc.ctx), rl_keys(bc.ctx), rl_keys_sorted(bc.ctx), rl_parent(bc.ctx), rl_keys32(bc.ctx), rl_rank(bc.ctx), rl_inv(bc.ctx),
          rl_tab(bc.ctx), rl_tmp(bc.ctx) {}

    int mark_fork()   // at the top of the build: everything enqueued on ctx->stream so far comes before the renumbering
    {
        if (!b.p.two_streams) return RK_OK;
        RK_TRY(ensure_stream2(b.ctx, b.k.stream2_high));
        RK_HIP(b.ctx, hipEventRecord(b.ctx->ev_fork, b.st));
        return RK_OK;
    }
    int join()   // ctx->stream waits for whatever the second stream was last given
    {
        if (!joined) {
            RK_HIP(b.ctx, hipStreamWaitEvent(b.st, b.ctx->ev_join, 0));
            joined = true;
        }
        return RK_OK;
    }
    // tile records need the translation table alone (sizes and offsets in internal order are still on their way on the second
    // stream: joined in front of the row sort)
    int wait_inv()
    {
        if (inv_recorded && !joined) RK_HIP(b.ctx, hipStreamWaitEvent(b.st, b.ctx->ev_inv, 0));
        else RK_TRY(join());
        return RK_OK;
    }
    int ensure_table()   // (second attempt: the renumbering ran for tile records, without k_emit_table's table)
    {
        if (!inv || rl_tab.p) return RK_OK;
        RK_HIP(b.ctx, rl_tab.alloc(b.p.N));
        hipLaunchKernelGGL(k_emit_table, dim3(blocks_for(b.p.N)), dim3(kThreads), 0, b.st, inv, b.idx->d_src_off, b.p.N, rl_tab.p);
        return RK_OK;
    }
    // the list heads of a one-pass build hang on the emission alone: they branch off to the second stream and are joined like the renumbering
    int branch_heads(hipStream_t *sh)
    {
        RK_HIP(b.ctx, hipEventRecord(b.ctx->ev_fork, b.st));
        RK_HIP(b.ctx, hipStreamWaitEvent(b.ctx->stream2, b.ctx->ev_fork, 0));
        *sh = b.ctx->stream2;
        return RK_OK;
    }
    int heads_branched()
    {
        RK_HIP(b.ctx, hipEventRecord(b.ctx->ev_join, b.ctx->stream2));
        joined = false;
        return RK_OK;
    }
    int enqueue(bool want_tab);
    int enqueue_identity();
};

// The launches of the renumbering are ENQUEUED after the partition's (the fast path calls this once its own first
// kernels are in the queue): the host needs ~5 us per launch, and with the renumbering's ten launches in front the
// partition started 70 us late.  want_tab: the fast path is taken with slice records and wants k_emit_table's table.
int Renumbering::enqueue(bool want_tab)
{
    if (enqueued) return RK_OK;
    enqueued = true;
    if (!b.p.relabel) return enqueue_identity();
    rk_ctx *ctx = b.ctx;
    rk_index *idx = b.idx;
    const BuildSource &src = b.src;
    const uint32_t N = b.p.N;
    hipStream_t s2 = b.st;
    if (b.p.two_streams) {
        s2 = ctx->stream2;
        RK_HIP(ctx, hipStreamWaitEvent(s2, ctx->ev_fork, 0));
        forked = true;
    }
    const int id_bits = b.p.gb;
    uint32_t slots = 1024;
    // (at most half full, usually far less -- relatives share their smallest hashes.  Twice this size was 268 MB at 500,000 genomes:
    // beyond the last-level cache, every probe a DRAM row of its own, and the kernels streaming beside it slowed to a third)
    const unsigned long long want_slots = b.k.table_x * N * kMinK;
    while (slots < want_slots && slots < (1u << 30)) slots <<= 1;
    RK_HIP(ctx, rl_table.alloc(slots));
    RK_HIP(ctx, rl_parent.alloc(N));
    RK_HIP(ctx, hipMemsetAsync(rl_table.p, 0xFF, (size_t)slots * 8, s2));
    const unsigned nb_ins = (unsigned)(((uint64_t)N * kMinK + kInsertThreads - 1) / kInsertThreads), nb_n = blocks_for(N);
    auto insert_and_vote = [&](auto rs) {   // rs: where a genome's smallest hashes are read
        using R = decltype(rs);
        hipLaunchKernelGGL(k_minhash_insert<R>, dim3(nb_ins), dim3(kInsertThreads), 0, s2, rs, N, rl_table.p, slots - 1);
        hipLaunchKernelGGL(k_minhash_vote<R>, dim3(nb_n), dim3(kThreads), 0, s2, rs, N, rl_table.p, slots - 1, rl_parent.p);
    };
    if (src.d_sig) insert_and_vote(SigMinK{src.d_sig});
    else if (idx->wide) insert_and_vote(CsrMinK<uint64_t>{src.s->d_hashes64, src.s->d_off});
    else insert_and_vote(CsrMinK<uint32_t>{src.s->d_hashes, src.s->d_off});
    if (N <= kRankMaxN) {
        RK_HIP(ctx, rl_keys32.alloc(N));
        RK_HIP(ctx, rl_rank.alloc(N));
        hipLaunchKernelGGL(k_cluster_keys32, dim3(nb_n), dim3(kThreads), 0, s2, rl_parent.p, N, id_bits, rl_keys32.p, rl_rank.p);
        hipLaunchKernelGGL(k_rank_keys, dim3((N + kRankQ - 1) / kRankQ, (N + kRankStretch - 1) / kRankStretch), dim3(kRankThreads), 0, s2,
                           rl_keys32.p, N, rl_rank.p);
        if (forked) {   // (a genome's rank among the keys IS its internal id: all the bucket emission of tile records needs)
            RK_HIP(ctx, hipEventRecord(ctx->ev_inv, s2));
            inv_recorded = true;
        }
        hipLaunchKernelGGL(k_order_from_rank, dim3(nb_n), dim3(kThreads), 0, s2, rl_rank.p, N, src.d_off, src.d_sizes, idx->d_orig, idx->d_sizes);
        hipLaunchKernelGGL(k_offsets_scan, dim3(1), dim3(1024), 0, s2, idx->d_sizes, N, idx->d_src_off);
        inv = rl_rank.p;   // (a genome's rank among the keys IS its internal id)
    } else {
        RK_HIP(ctx, rl_keys.alloc(N));
        RK_HIP(ctx, rl_keys_sorted.alloc(N));
        RK_HIP(ctx, rl_inv.alloc(N));
        hipLaunchKernelGGL(k_cluster_keys, dim3(nb_n), dim3(kThreads), 0, s2, rl_parent.p, N, id_bits, rl_keys.p);
        void *scratch = nullptr;
        RK_TRY(rk_prim_sort_keys_u64(ctx, rl_keys.p, rl_keys_sorted.p, N, 0, (unsigned)(2 * id_bits), s2, &scratch));
        rl_tmp.p = static_cast<char *>(scratch);
        hipLaunchKernelGGL(k_order_from_keys, dim3(nb_n), dim3(kThreads), 0, s2, rl_keys_sorted.p, N, id_bits, src.d_off, src.d_sizes, idx->d_orig, idx->d_sizes);
        hipLaunchKernelGGL(k_invert_order, dim3(nb_n), dim3(kThreads), 0, s2, idx->d_orig, N, rl_inv.p);
        if (forked) {   // (the translation table is all the bucket emission of tile records needs: it need not wait for the offsets' scan)
            RK_HIP(ctx, hipEventRecord(ctx->ev_inv, s2));
            inv_recorded = true;
        }
        hipLaunchKernelGGL(k_offsets_scan, dim3(1), dim3(1024), 0, s2, idx->d_sizes, N, idx->d_src_off);
        inv = rl_inv.p;
    }
    if (want_tab) {
        RK_HIP(ctx, rl_tab.alloc(N));
        hipLaunchKernelGGL(k_emit_table, dim3(nb_n), dim3(kThreads), 0, s2, inv, idx->d_src_off, N, rl_tab.p);
    }
    if (idx->d_blk_min) hipLaunchKernelGGL(k_blk_min_sizes, dim3(blocks_for(b.p.n_blocks)), dim3(kThreads), 0, s2, idx->d_sizes, N, b.p.n_blocks, idx->d_blk_min);
    idx->relabeled = true;
    RK_HIP(ctx, hipGetLastError());
    if (forked) {
        RK_HIP(ctx, hipEventRecord(ctx->ev_join, s2));
        joined = false;
    }
    return RK_OK;
}
int Renumbering::enqueue_identity()   // no renumbering: the caller's order, on the context's stream
{
    rk_index *idx = b.idx;
    const uint32_t N = b.p.N;
    hipLaunchKernelGGL(k_iota, dim3(blocks_for((uint64_t)N + 1)), dim3(kThreads), 0, b.st, N, idx->d_orig);
    if (b.src.d_sizes) {
        RK_HIP(b.ctx, hipMemcpyAsync(idx->d_sizes, b.src.d_sizes, (size_t)N * 4, hipMemcpyDeviceToDevice, b.st));
        hipLaunchKernelGGL(k_offsets_scan, dim3(1), dim3(1024), 0, b.st, idx->d_sizes, N, idx->d_src_off);
    } else {
        hipLaunchKernelGGL(k_sizes, dim3(blocks_for((uint64_t)N + 1)), dim3(kThreads), 0, b.st, b.src.d_off, N, idx->d_sizes, idx->d_src_off);
    }
    if (idx->d_blk_min) hipLaunchKernelGGL(k_blk_min_sizes, dim3(blocks_for(b.p.n_blocks)), dim3(kThreads), 0, b.st, idx->d_sizes, N, b.p.n_blocks, idx->d_blk_min);
    return RK_OK;
}

// ---- fast path: two-level bucket sort, second level and all emission in LDS (rk_index_fast.inc) -----------------
// the temporaries of one attempt
struct AttemptBufs {
    DevBuf<uint32_t> chunk_first, matrix, total, bstart, ucount, ubase, tmp_uhash, tmp_upos, n_open, n_cov, big_list;
    DevBuf<unsigned long long> keys, mid, tmp_uhash64, zeroed;
    DevBuf<uint2> self_raw;
    DevBuf<uint3> t_rec;   // the unsorted tile records (64 regions); a shard's: grouped by destination shard (they leave for the exchange unsorted)
    TileSortBufs sort;
    ZeroedLayout z;
    explicit AttemptBufs(rk_ctx *c)
        : chunk_first(c), matrix(c), total(c), bstart(c), ucount(c), ubase(c), tmp_uhash(c), tmp_upos(c), n_open(c), n_cov(c), big_list(c), keys(c), mid(c),
          tmp_uhash64(c), zeroed(c), self_raw(c), t_rec(c), sort(c) {}
};
inline size_t part_lds_bytes(uint32_t nb) { return (size_t)nb * 4 + 2 * kStageGenomes * 8; }   // bucket counters + the chunk's genome bounds

// allocates an attempt's buffers, lays out `zeroed` and zeroes it (k_chunk_first, the first launch)
int begin_attempt(const BuildCtx &b, const AttemptPlan &a, AttemptBufs &m)
{
    rk_ctx *ctx = b.ctx;
    const BuildPlan &p = b.p;
    const size_t nb1 = (size_t)a.nb + 1;
    RK_HIP(ctx, m.chunk_first.alloc((size_t)a.n_chunks + 1));
    RK_HIP(ctx, m.matrix.alloc((size_t)a.part_chunks * a.nb));
    RK_HIP(ctx, m.total.alloc(a.nb));
    RK_HIP(ctx, m.bstart.alloc(nb1 * a.passes));   // (per pass: the list heads of a pass are placed while the next one partitions)
    RK_HIP(ctx, m.ucount.alloc(nb1 * a.passes));
    RK_HIP(ctx, m.ubase.alloc(nb1 * a.passes));
    if (p.wide) RK_HIP(ctx, m.tmp_uhash64.alloc(p.H_el));
    else RK_HIP(ctx, m.tmp_uhash.alloc(p.H_el));
    RK_HIP(ctx, m.tmp_upos.alloc(p.H_el));
    RK_HIP(ctx, m.keys.alloc(a.keys_cap));
    if (a.tiles_mode) RK_HIP(ctx, m.t_rec.alloc(a.rec_cap));
    if (a.sort_here) RK_TRY(m.sort.alloc(ctx, p.n_blocks, a.rec_cap, std::min<uint64_t>(a.rec_cap, (uint64_t)p.n_blocks * (p.n_blocks + 1) / 2)));
    if (!a.tiles_mode) {
        RK_HIP(ctx, m.self_raw.alloc(p.H));
        RK_HIP(ctx, m.n_open.alloc((size_t)p.N + 1));
        RK_HIP(ctx, m.n_cov.alloc((size_t)p.N + 1));
    }
    m.z = ZeroedLayout::of_build(a.passes, a.part2, a.small_wgs, a.nb, a.n_chunks, a.sort_here, p.n_blocks);
    RK_HIP(ctx, m.zeroed.alloc(m.z.z_end));
    m.z.base = m.zeroed.p;
    const size_t part_lds = part_lds_bytes(a.nb);
    if (part_lds > 48 * 1024) {
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_part_hist<uint32_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part_lds));
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_part_scatter<uint32_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part_lds));
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_part_hist<uint64_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part_lds));
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_part_scatter<uint64_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part_lds));
    }
    // (from keys: no chunk walks the sketches -- the launch only zeroes, and chunk_first[0] is all it writes)
    hipLaunchKernelGGL(k_chunk_first, dim3(blocks_for(std::max<uint64_t>((uint64_t)a.n_chunks + 1, m.z.z_end))), dim3(kThreads), 0, b.st, b.src.d_off, p.N,
                       p.from_keys ? 0u : a.n_chunks, m.chunk_first.p, m.zeroed.p, (uint32_t)m.z.z_end);
    if (a.part2) RK_HIP(ctx, m.mid.alloc(a.keys_cap));
    if (a.big_ok) {
        RK_HIP(ctx, m.big_list.alloc((size_t)a.nb * a.passes));
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_bucket_heavy<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)heavy_lds_bytes(p.n_blocks)));
    }
    return RK_OK;
}

// what the kernels that walk the sketches see of an attempt (range_id: per pass)
FastArgs fast_args(const BuildCtx &b, const AttemptPlan &a)
{
    const BuildPlan &p = b.p;
    FastArgs fa;
    fa.hashes = p.from_keys ? nullptr : p.wide ? (const void *)b.src.s->d_hashes64 : (const void *)b.src.s->d_hashes;
    fa.off = b.src.d_off;
    fa.orig = nullptr;           // the partition walks the sketches in the caller's order (see the renumbering above)
    fa.off_new = b.src.d_off;
    fa.n_genomes = p.N;
    fa.H = p.H_el;
    fa.hash_bits = p.hash_bits;
    fa.low_bits = p.low_bits;
    fa.gb = p.gb;
    fa.rb = a.rb;
    fa.xcd_map = b.k.xcd_map;
    fa.nb = a.nb;
    fa.n_chunks = a.n_chunks;
    fa.range_bits = a.range_bits;
    fa.range_id = 0;
    fa.keys_cap = a.keys_cap;
    fa.filtered = nullptr;
    fa.n_filtered = nullptr;
    return fa;
}

// one pass's partition: filter -> hist -> colscan -> starts -> coarse + fine, or scatter.  The pass's keys lie in m.keys, bucket by bucket.
int launch_partition_pass(const BuildCtx &b, const AttemptPlan &a, AttemptBufs &m, FastArgs fa, uint32_t pass)
{
    rk_ctx *ctx = b.ctx;
    const BuildPlan &p = b.p;
    hipStream_t st = b.st;
    BuildResult *const fres = m.z.res();
    uint32_t *const bstart_p = m.bstart.p + ((size_t)a.nb + 1) * pass;
    const size_t part_lds = part_lds_bytes(a.nb);
    fa.range_id = (p.shard_id << p.pass_bits) | pass;
    FastArgs pa = fa;   // what the partition kernels of this pass see
    if (a.use_filter) {
        unsigned long long *const n_filt = m.z.n_filtered(pass);
        pa.filtered = m.keys.p;
        if (p.from_keys && a.passes == 1) {
            // the caller's keys are never written: one pass partitions them as they are (k_part_fine writes `keys`, ours), several
            // passes filter them into `keys` first -- a second attempt (tile records beyond their buffer) starts from intact keys
            hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(64), 0, st, n_filt, (unsigned long long)p.H_el);
            pa.filtered = b.src.keys;
        } else if (p.from_keys) {
            const uint64_t per_wg = (uint64_t)kKeysFilterThreads * kKeysFilterSteps;
            if (p.H_el)
                hipLaunchKernelGGL(k_keys_pass_filter, dim3((unsigned)((p.H_el + per_wg - 1) / per_wg)), dim3(kKeysFilterThreads), 0, st, b.src.keys, p.H_el, p.gb,
                                   p.hash_bits - p.shard_bits, p.pass_bits, pass, m.keys.p, n_filt, (unsigned long long)a.keys_cap, fres);
        } else {
            // (the filtered elements lie in `keys`: the coarse pass reads them and writes `mid`, the fine pass writes `keys` again)
            RK_TRY(with_hash_type(p.wide, [&](auto ht) -> int {
                hipLaunchKernelGGL(k_range_filter<decltype(ht)>, dim3(fa.n_chunks * kFilterSplit), dim3(kFilterThreads), 0, st, fa, m.chunk_first.p, m.keys.p, n_filt, fres);
                return RK_OK;
            }));
            // (tried: starting the renumbering BEHIND the filter -- then k_part_hist takes 0.84 ms instead of 0.16 beside
            // k_minhash_insert: whatever runs beside that kernel pays its 0.55 ms)
        }
        pa.n_filtered = n_filt;
        pa.hash_bits = p.eff_bits;
        pa.range_bits = 0;
        pa.range_id = 0;
    }
    RK_TRY(with_hash_type(p.wide, [&](auto ht) -> int {
        hipLaunchKernelGGL(k_part_hist<decltype(ht)>, dim3(a.part_chunks), dim3(kPartThreads), part_lds, st, pa, m.chunk_first.p, m.matrix.p, fres);
        return RK_OK;
    }));
    hipLaunchKernelGGL(k_part_colscan, dim3((a.nb + 63) / 64), dim3(1024), 0, st, m.matrix.p, a.part_chunks, a.nb, m.total.p);
    hipLaunchKernelGGL(k_part_starts, dim3(1), dim3(1024), 0, st, m.total.p, a.nb, bstart_p, fres, m.z.pass_base() + pass, (unsigned long long)a.keys_cap,
                       a.big_ok ? m.big_list.p + (size_t)a.nb * pass : nullptr, m.z.n_big(pass));
    // the partition itself: two coalescing passes (rk_index_fast.inc), or one scattering pass
    return with_hash_type(p.wide, [&](auto ht) -> int {
        using HT = decltype(ht);
        if (!a.part2) {
            hipLaunchKernelGGL(k_part_scatter<HT>, dim3(fa.n_chunks), dim3(kPartThreads), part_lds, st, fa, m.chunk_first.p, m.matrix.p, bstart_p, m.keys.p, fres);
            return RK_OK;
        }
        auto coarse = [&](auto t, unsigned grid) -> int {
            constexpr uint32_t TT = decltype(t)::value;
            RK_HIP(ctx, hipFuncSetAttribute((const void *)k_part_coarse<TT, HT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part2_lds(TT)));
            hipLaunchKernelGGL((k_part_coarse<TT, HT>), dim3(grid), dim3(TT), part2_lds(TT), st, pa, m.chunk_first.p, m.matrix.p, bstart_p, m.z.seg_taken(pass), m.mid.p, fres);
            return RK_OK;
        };
        RK_TRY(a.small_wgs ? coarse(Threads<256>(), a.part_chunks * 4) : coarse(Threads<1024>(), a.part_chunks));
        hipLaunchKernelGGL(k_part_fine, dim3(a.nb >> kFineBits, 16), dim3(kPartThreads), 0, st, pa, bstart_p, m.mid.p, m.keys.p, m.z.fine_cursor(pass), fres);
        return RK_OK;
    });
}

// one pass's emission out of the sorted buckets: tile or slice records (+ the heavy buckets), then the list heads
int launch_emit_pass(const BuildCtx &b, Renumbering &rn, const AttemptPlan &a, AttemptBufs &m, uint32_t pass)
{
    rk_ctx *ctx = b.ctx;
    const BuildPlan &p = b.p;
    rk_index *idx = b.idx;
    hipStream_t st = b.st;
    const size_t nb1 = (size_t)a.nb + 1;
    uint32_t *const bstart_p = m.bstart.p + nb1 * pass, *const ucount_p = m.ucount.p + nb1 * pass, *const ubase_p = m.ubase.p + nb1 * pass;
    BuildResult *const fres = m.z.res();
    unsigned long long *const pass_base = m.z.pass_base() + pass;
    auto fill_common = [&](auto &ea) {   // what EmitArgs and TileEmitArgs share
        ea.keys = m.keys.p;
        ea.bstart = bstart_p;
        ea.inv = rn.inv;
        ea.low_bits = p.low_bits;
        ea.gb = p.gb;
        ea.rb = a.rb;
        ea.nb = a.nb;
        ea.postings = idx->d_postings;
        ea.tmp_uhash = m.tmp_uhash.p;
        ea.tmp_uhash64 = p.wide ? m.tmp_uhash64.p : nullptr;
        ea.tmp_upos = m.tmp_upos.p;
        ea.ucount = ucount_p;
        ea.xcd_map = b.k.xcd_map;
        ea.debug = b.k.debug;
    };
    if (b.k.debug) {  // developer ablations leave stages out: whatever they do not write must still be harmless downstream
        RK_HIP(ctx, hipMemsetAsync(ucount_p, 0, (size_t)a.nb * 4, st));
        if (!a.tiles_mode) RK_HIP(ctx, hipMemsetAsync(m.self_raw.p, 0, p.H * sizeof(uint2), st));
        RK_HIP(ctx, hipMemsetAsync(m.tmp_upos.p, 0, p.H_el * 4, st));
    }
    if (a.tiles_mode) {
        TileEmitArgs ea;
        fill_common(ea);
        ea.rec = m.t_rec.p;
        ea.region_cap = a.region_cap;
        ea.pass_base = pass_base;
        ea.hash_base = a.range_bits ? ((unsigned long long)((p.shard_id << p.pass_bits) | pass) << p.eff_bits) : 0ULL;
        ea.n_dest = p.n_shards;
        ea.stop = a.range_bits ? fres : nullptr;
        ea.big_ok = a.big_ok ? 1 : 0;
        ea.big_list = a.big_ok ? m.big_list.p + (size_t)a.nb * pass : nullptr;
        ea.n_big = m.z.n_big(pass);
        ea.stop_rw = fres;
        ea.tres = m.z.tile_res();
        RK_TRY(with_emit_shape(b.k.emit_t, a.narrow, [&](auto t, auto key) -> int {
            hipLaunchKernelGGL((k_bucket_emit_tiles<decltype(t)::value, decltype(key)>), dim3(a.nb), dim3(decltype(t)::value), 0, st, ea);
            return RK_OK;
        }));
        if (a.big_ok) {
            HeavyArgs ha;
            ha.e = ea;
            ha.big_list = ea.big_list;
            ha.n_big = ea.n_big;
            ha.next = m.z.heavy_next(pass);
            ha.n_blocks = p.n_blocks;
            hipLaunchKernelGGL(k_bucket_heavy<1024>, dim3((unsigned)std::max(1, ctx->num_cu)), dim3(1024), heavy_lds_bytes(p.n_blocks), st, ha);
        }
    } else {
        EmitArgs ea;
        fill_common(ea);
        ea.off_new = idx->d_src_off;
        ea.tab = rn.inv ? rn.rl_tab.p : nullptr;
        ea.self_raw = m.self_raw.p;
        ea.res = fres;
        RK_TRY(with_emit_shape(b.k.emit_t, a.narrow, [&](auto t, auto key) -> int {
            hipLaunchKernelGGL((k_bucket_emit<decltype(t)::value, decltype(key)>), dim3(a.nb), dim3(decltype(t)::value), 0, st, ea);
            return RK_OK;
        }));
    }
    // the list heads (scan + placement) hang on the emission alone: they go to the second stream (one pass) and run beside
    // the rows / the tile sort; with several passes they stay in line (the next pass's partition is the bigger job)
    hipStream_t sh = st;
    const bool heads_aside = rn.forked && a.passes == 1;
    if (heads_aside) RK_TRY(rn.branch_heads(&sh));
    hipLaunchKernelGGL(k_heads_scan, dim3(1), dim3(1024), 0, sh, ucount_p, a.nb, ubase_p, fres);
    RK_TRY(with_key_type(!p.wide, [&](auto h) -> int {   // (the list heads' hashes: 32 bits, or the 64-bit layout)
        using HT = decltype(h);
        hipLaunchKernelGGL(k_heads_place<HT>, dim3(a.nb), dim3(kThreads), 0, sh, p.wide ? (const HT *)m.tmp_uhash64.p : (const HT *)m.tmp_uhash.p, m.tmp_upos.p, bstart_p,
                           ucount_p, ubase_p, a.nb, pass_base, p.wide ? (HT *)idx->d_uhash64 : (HT *)idx->d_uhash, idx->d_upos);
        return RK_OK;
    }));
    if (heads_aside) RK_TRY(rn.heads_branched());
    return RK_OK;
}

// (developer output: what k_bucket_heavy had to take)
int report_heavy(const BuildCtx &b, const AttemptPlan &a, const AttemptBufs &m)
{
    rk_ctx *ctx = b.ctx;
    const size_t nb1 = (size_t)a.nb + 1;
    std::vector<uint32_t> nbig(a.passes), bs(nb1 * a.passes);
    RK_TRY(rk_read_back(ctx, nbig.data(), m.z.n_big(0), (size_t)a.passes * 4, b.st));
    RK_TRY(rk_read_back(ctx, bs.data(), m.bstart.p, bs.size() * 4, b.st));
    for (uint32_t pass = 0; pass < a.passes; pass++) {
        std::vector<uint32_t> bl(nbig[pass]);
        if (nbig[pass]) RK_TRY(rk_read_back(ctx, bl.data(), m.big_list.p + (size_t)a.nb * pass, bl.size() * 4, b.st));
        unsigned long long keys_in = 0, biggest = 0;
        for (uint32_t bk : bl) {
            const unsigned long long n = bs[nb1 * pass + bk + 1] - bs[nb1 * pass + bk];
            keys_in += n;
            biggest = std::max(biggest, n);
        }
        fprintf(stderr, "[rk] index build pass %u: %u of %u buckets for k_bucket_heavy, %llu keys, biggest %llu\n", pass, nbig[pass], a.nb, keys_in, biggest);
    }
    return RK_OK;
}

// How an attempt of the bucket sort ended.
struct AttemptOutcome {
    enum What {
        Built,
        RetryKeysCap,       // a range pass holds `need` keys, more than estimated: once more with buffers for them
        RetryRecCap,        // the tile records did not fit: once more with room for the `need` the attempt counted
        FallBackToSlices,   // ... beyond the budget of tile records: slice records after all
        Refused             // the kernels raised `flags`, or (flags == 0) the tile records overflowed with no way on: the general path decides
    } what;
    unsigned long long need, flags;
    unsigned long long heavy;   // buckets the attempt handed to k_bucket_heavy, summed over its passes
    uint32_t passes;
    BuildResult r;
    TileResult tr;
};

// (the tile records of an attempt did not fit their buffer -- wide species, lists scattered over many blocks --: the
// attempt has counted what it needs, and the next one gets exactly that, within a budget of 6 records per posting; beyond
// it the index is built with slice records after all, where those can be had)
void after_tile_overflow(const BuildCtx &b, const RetryState &rs, AttemptOutcome *o)
{
    unsigned long long worst = 0;
    for (uint32_t q = 0; q < kRecRegions; q++) worst = std::max<unsigned long long>(worst, o->tr.rec_count[q]);
    o->need = (worst + worst / 16 + 1024) * kRecRegions;
    if (!rs.rec_cap_retry && o->need <= 6 * b.p.H_el_shard + (1u << 22) && !b.ctx->sw_tile_rec_cap) o->what = AttemptOutcome::RetryRecCap;   // (RK_TILE_REC_CAP: a test forces the fallback)
    else o->what = b.p.slices_ok ? AttemptOutcome::FallBackToSlices : AttemptOutcome::Refused;
}

// One attempt of the bucket sort: allocate, partition and emit pass by pass, the tile sort or the rows, ONE synchronising read-back.
int bucket_sort_attempt(const BuildCtx &b, Renumbering &rn, const RetryState &rs, AttemptOutcome *o)
{
    rk_ctx *ctx = b.ctx;
    const BuildPlan &p = b.p;
    rk_index *idx = b.idx;
    hipStream_t st = b.st;
    AttemptPlan a;
    RK_TRY(plan_attempt(ctx, p, b.k, rs, &a));
    if (!a.tiles_mode) RK_TRY(alloc_slices(ctx, idx, p));
    AttemptBufs m(ctx);
    RK_TRY(begin_attempt(b, a, m));
    const FastArgs fa = fast_args(b, a);
    for (uint32_t pass = 0; pass < a.passes; pass++) {
        RK_TRY(launch_partition_pass(b, a, m, fa, pass));
        if (pass == 0) {
            RK_TRY(rn.enqueue(!a.tiles_mode));   // (behind the partition's launches in the host's queue, beside them on the device)
            // the internal order is needed from here on: the translation table alone for tile records, everything for slice records
            if (a.tiles_mode) RK_TRY(rn.wait_inv());
            else {
                RK_TRY(rn.join());
                RK_TRY(rn.ensure_table());
            }
        }
        RK_TRY(launch_emit_pass(b, rn, a, m, pass));
    }
    BuildResult *const fres = m.z.res();
    if (a.sort_here) {
        RK_TRY(launch_tile_sort(ctx, m.sort.args(m.t_rec.p, a.region_cap, p.n_blocks, idx->d_blk_min, m.z), st, [&]() { return rn.join(); }));
    } else if (!a.tiles_mode) {
        const unsigned wave_blocks = (p.N + 3) / 4;  // 4 waves (genomes) per 256-thread workgroup
        hipLaunchKernelGGL(k_row_counts2, dim3(wave_blocks), dim3(kThreads), 0, st, idx->d_src_off, p.N, m.self_raw.p, m.n_open.p, m.n_cov.p);
        hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(1024), 0, st, m.n_open.p, m.n_cov.p, p.N, idx->d_self_off, idx->d_self_split, fres);
        hipLaunchKernelGGL(k_row_place2, dim3(wave_blocks), dim3(kThreads), 0, st, idx->d_src_off, p.N, m.self_raw.p, idx->d_self_off,
                           idx->d_self_split, idx->d_selfrange);
    }
    RK_HIP(ctx, hipGetLastError());
    RK_TRY(rn.join());
    unsigned long long n_postings = 0;
    {   // the one synchronisation of the build: both result records, the postings of all passes and -- they lie directly behind, for
        // rk_index_build_report -- the passes' counts of buckets for k_bucket_heavy (n_big[]) in one read-back
        struct { BuildResult r; TileResult t; unsigned long long pass_base[257 + 128]; } both;
        static_assert(sizeof(BuildResult) % 8 == 0 && offsetof(decltype(both), pass_base) == sizeof(BuildResult) + sizeof(TileResult), "the records lie back to back");
        const size_t big_at = m.z.z_big - m.z.z_pass, words = m.z.z_filt - m.z.z_pass;   // (ZeroedLayout: passes + 1 words, then a u32 per pass; at most 256 passes)
        RK_TRY(rk_read_back(ctx, &both, fres, sizeof(BuildResult) + sizeof(TileResult) + words * 8, st));
        o->r = both.r;
        o->tr = both.t;
        n_postings = both.pass_base[a.passes];
        o->heavy = 0;
        o->passes = a.passes;
        for (uint32_t pass = 0; pass < a.passes; pass++) {
            uint32_t n_big;
            memcpy(&n_big, reinterpret_cast<const char *>(&both.pass_base[big_at]) + (size_t)pass * 4, 4);
            o->heavy += n_big;
        }
    }
    const BuildResult &r = o->r;
    const TileResult &tr = o->tr;
    if (ctx->sw_dist_debug && a.big_ok) RK_TRY(report_heavy(b, a, m));
    if (ctx->sw_dist_debug)
        fprintf(stderr, "[rk] index build: fast path flags %llu (B %d, low bits %d, genome bits %d, position bits %d; shard %u of %u, %u pass(es), %llu postings)%s\n",
                r.flags, p.B, p.low_bits, p.gb, p.rb, p.shard_id, p.n_shards, a.passes, n_postings, a.tiles_mode ? (tr.overflow ? ", tile records overflowed" : ", tile records") : "");
    o->need = 0;
    o->flags = r.flags;
    if ((r.flags & kFastOverflow) && a.use_filter && !p.from_keys && !rs.keys_cap_retry) {
        // a range holds more keys than estimated: every pass's filter has counted what it needs -- once more with exactly that
        std::vector<unsigned long long> asked(a.passes);
        RK_TRY(rk_read_back(ctx, asked.data(), m.z.n_filtered(0), (size_t)a.passes * 8, st));
        o->need = *std::max_element(asked.begin(), asked.end());
        if (o->need > a.keys_cap && o->need <= p.H) {
            if (ctx->sw_dist_debug) fprintf(stderr, "[rk] index build: a range pass holds %llu keys (buffers for %llu): again\n", o->need, (unsigned long long)a.keys_cap);
            o->what = AttemptOutcome::RetryKeysCap;
            return RK_OK;
        }
    }
    if (r.flags) {   // a bucket beyond the LDS sort, a pass beyond its key buffer, or a hash outside the hash space
        o->what = AttemptOutcome::Refused;
        return RK_OK;
    }
    if (a.tiles_mode && tr.overflow) {
        after_tile_overflow(b, rs, o);
        return RK_OK;
    }
    o->what = AttemptOutcome::Built;
    if (p.range_bits) idx->H = n_postings;   // (a shard: the postings of ITS hash range; all passes of one shard: == H)
    if (a.sort_here) {
        m.sort.hand_over(idx, tr);
        if (ctx->sw_dist_debug)
            fprintf(stderr, "[rk] tiles from the build: %llu tiles, %llu records in %llu slots (capacity %llu), biggest tile %llu\n", tr.n_tiles, tr.n_records,
                    tr.n_slots, (unsigned long long)a.rec_cap, tr.max_records);
    }
    if (a.tiles_mode && p.n_shards > 1) {   // the shard's records wait for the exchange (rk_index_shard_records / _pack)
        idx->d_shard_rec = m.t_rec.release();
        idx->shard_region_cap = a.region_cap;
        idx->n_shards = p.n_shards;
        idx->shard_id = p.shard_id;
        for (uint32_t q = 0; q < kRecRegions; q++) idx->shard_rec_count[q] = tr.rec_count[q];
    }
    return RK_OK;
}

// ---- general path: device-wide stable radix sort of (hash, source element) -------------------------------------
int build_general(const BuildCtx &b, BuildResult *res, BuildResult *r)
{
    rk_ctx *ctx = b.ctx;
    rk_index *idx = b.idx;
    const rk_sketches *s = b.src.s;
    hipStream_t st = b.st;
    const uint64_t H = b.p.H;
    const uint32_t N = b.p.N;
    const bool no_self = b.p.no_self;
    const unsigned wave_blocks = (N + 3) / 4;  // 4 waves (genomes) per 256-thread workgroup
    RK_HIP(ctx, hipMemsetAsync(res, 0, sizeof(BuildResult), st));
    const void *src_hashes = idx->wide ? (const void *)s->d_hashes64 : (const void *)s->d_hashes;
    const uint64_t *src_off = s->d_off;
    DevBuf<char> perm_hashes(ctx);
    if (idx->relabeled) {  // the sketches in internal order
        RK_HIP(ctx, perm_hashes.alloc(H * (idx->wide ? 8 : 4)));
        RK_TRY(with_hash_type(idx->wide, [&](auto ht) -> int {
            using HT = decltype(ht);
            hipLaunchKernelGGL(k_gather_sketches<HT>, dim3(wave_blocks), dim3(kThreads), 0, st, (const HT *)src_hashes, s->d_off, idx->d_orig,
                               idx->d_src_off, N, (HT *)perm_hashes.p);
            return RK_OK;
        }));
        src_hashes = perm_hashes.p;
        src_off = idx->d_src_off;
    }
    DevBuf<uint32_t> iota(ctx), sorted_e(ctx), flags(ctx), gid(ctx), n_open(ctx), n_cov(ctx);
    DevBuf<char> keys_sorted(ctx);
    DevBuf<uint2> self_raw(ctx);
    RK_HIP(ctx, iota.alloc(H));
    RK_HIP(ctx, sorted_e.alloc(H));
    RK_HIP(ctx, flags.alloc(H));
    RK_HIP(ctx, gid.alloc(H));
    RK_HIP(ctx, self_raw.alloc(no_self ? 1 : H));
    RK_HIP(ctx, n_open.alloc((size_t)N + 1));
    RK_HIP(ctx, n_cov.alloc((size_t)N + 1));
    RK_HIP(ctx, keys_sorted.alloc(H * (idx->wide ? 8 : 4)));
    hipLaunchKernelGGL(k_fill_gid, dim3(wave_blocks), dim3(kThreads), 0, st, src_off, N, gid.p, iota.p);
    uint32_t *gidx = iota.p;  // (after the scan) 1-based group number of each sorted position
    // stable LSD radix sort by hash; values = source element index (genome-major), so equal hashes stay in
    // ascending genome order == hashMapId[hash].push_back(i) for i ascending (src/sketch.cpp:979-985)
    if (idx->wide) RK_TRY(rk_prim_sort_pairs_u64_u32(ctx, (const uint64_t *)src_hashes, (uint64_t *)keys_sorted.p, iota.p, sorted_e.p, H, (unsigned)b.p.hash_bits, st));
    else RK_TRY(rk_prim_sort_pairs_u32_u32(ctx, (const uint32_t *)src_hashes, (uint32_t *)keys_sorted.p, iota.p, sorted_e.p, H, (unsigned)b.p.hash_bits, st));
    RK_TRY(with_hash_type(idx->wide, [&](auto ht) -> int {
        using HT = decltype(ht);
        hipLaunchKernelGGL(k_head_flags<HT>, dim3(blocks_for(H)), dim3(kThreads), 0, st, (const HT *)keys_sorted.p, H, flags.p);
        RK_TRY(rk_prim_inclusive_scan_u32(ctx, flags.p, iota.p, H, st));
        hipLaunchKernelGGL(k_scatter_heads<HT>, dim3(blocks_for(H)), dim3(kThreads), 0, st, (const HT *)keys_sorted.p, gidx, H,
                           idx->wide ? (HT *)idx->d_uhash64 : (HT *)idx->d_uhash, idx->d_upos, res);
        return RK_OK;
    }));
    if (no_self)
        hipLaunchKernelGGL((k_postings_selfrange<false, true>), dim3(blocks_for(H)), dim3(kThreads), 0, st, sorted_e.p, gidx,
                           idx->d_upos, gid.p, H, idx->d_postings, self_raw.p, res);
    else if (s->is_set)
        hipLaunchKernelGGL(k_postings_selfrange<false>, dim3(blocks_for(H)), dim3(kThreads), 0, st, sorted_e.p, gidx,
                           idx->d_upos, gid.p, H, idx->d_postings, self_raw.p, res);
    else
        hipLaunchKernelGGL(k_postings_selfrange<true>, dim3(blocks_for(H)), dim3(kThreads), 0, st, sorted_e.p, gidx,
                           idx->d_upos, gid.p, H, idx->d_postings, self_raw.p, res);
    if (!no_self) {
        // drop the empty slices (26 % of the elements at 10,000 genomes), covered slices last in their row
        hipLaunchKernelGGL(k_row_counts, dim3(wave_blocks), dim3(kThreads), 0, st, src_off, N, self_raw.p, n_open.p, n_cov.p);
        hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(1024), 0, st, n_open.p, n_cov.p, N, idx->d_self_off, idx->d_self_split, res);
        hipLaunchKernelGGL(k_row_place, dim3(wave_blocks), dim3(kThreads), 0, st, src_off, N, self_raw.p,
                           idx->d_self_off, idx->d_self_split, idx->d_postings, s->is_set, idx->d_selfrange);
    }
    RK_HIP(ctx, hipGetLastError());
    return rk_read_back(ctx, r, res, sizeof(*r), st);  // the one synchronisation of the build
}
// no postings at all: empty lists, empty rows
int build_empty(const BuildCtx &b)
{
    RK_HIP(b.ctx, hipMemsetAsync(b.idx->d_upos, 0, 8, b.st));
    if (!b.p.no_self) {
        RK_HIP(b.ctx, hipMemsetAsync(b.idx->d_self_off, 0, ((size_t)b.p.N + 1) * 8, b.st));
        RK_HIP(b.ctx, hipMemsetAsync(b.idx->d_self_split, 0, ((size_t)b.p.N + 1) * 8, b.st));
    }
    RK_HIP(b.ctx, hipStreamSynchronize(b.st));
    return RK_OK;
}

int index_build_impl(rk_ctx *ctx, const BuildSource &src, int hash_bits, uint32_t shard_id, uint32_t n_shards, rk_index **out)
{
    if (!ctx || !out) return RK_ERR_ARG;
    *out = nullptr;
    const BuildKnobs k = read_knobs();
    BuildPlan p;
    RK_TRY(plan_build(ctx, src, hash_bits, shard_id, n_shards, k, &p));
    RK_HIP(ctx, hipSetDevice(ctx->device));
    rk_index *idx = new (std::nothrow) rk_index;
    if (!idx) return RK_ERR_NOMEM;
    idx->ctx = ctx;
    idx->n_ref = p.N;
    idx->H = p.H;
    idx->hash_bits = hash_bits;
    idx->wide = src.wide;
    idx->max_src_size = idx->max_ref_size = src.max_size;
    idx->min_ref_size = src.min_size;
    IndexGuard guard{idx};
    RK_TRY(alloc_index_arrays(ctx, idx, p));
    const BuildCtx b{ctx, src, p, k, idx, ctx->stream};
    Renumbering rn(b);
    RK_TRY(rn.mark_fork());
    DevBuf<BuildResult> res(ctx);   // the general path's result record
    RK_HIP(ctx, res.alloc(1));
    if (ctx->sw_dist_debug && !p.fast_ok())
        fprintf(stderr, "[rk] index build: general path (H %llu, wide %d, sets %d, B %d, low bits %d, genome bits %d, position bits %d)\n",
                (unsigned long long)p.H, (int)idx->wide, (int)src.is_set, p.B, p.low_bits, p.gb, p.rb);

    // the bucket sort: at most one retry with bigger key buffers, one with room for more tile records, then slice records
    RetryState rs{p.tiles_mode};
    AttemptOutcome o;
    memset(&o, 0, sizeof o);
    o.what = AttemptOutcome::Refused;
    uint64_t *const rep = idx->build_report;   // rk_index_build_report
    for (bool again = p.fast_ok(); again;) {
        RK_TRY(bucket_sort_attempt(b, rn, rs, &o));
        rep[RK_REPORT_ATTEMPTS]++;
        switch (o.what) {
        case AttemptOutcome::RetryKeysCap:
            rs.keys_cap_retry = o.need + o.need / 64 + 65536;
            rep[RK_REPORT_KEY_RETRIES]++;
            break;
        case AttemptOutcome::RetryRecCap:
            rs.rec_cap_retry = o.need;
            rep[RK_REPORT_REC_RETRIES]++;
            break;
        case AttemptOutcome::FallBackToSlices:
            rs.tiles_mode = false;
            drop_blk_min(ctx, idx);
            rep[RK_REPORT_FELL_BACK] = 1;
            break;
        default: again = false;
        }
    }
    rep[RK_REPORT_FLAGS] = o.flags;
    rep[RK_REPORT_HEAVY] = o.heavy;
    rep[RK_REPORT_PASSES] = o.passes;
    const bool built = o.what == AttemptOutcome::Built;
    if (!built && p.from_keys && (o.flags & kFastBadHash))
        return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_shard_keys: a key outside the wire format (hash bits beyond the shard's range, or a genome id >= %u)", p.N);
    if (!built && n_shards > 1)
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_index_build_shard: the bucket sort refused this collection (flags %s: a bucket or a pass beyond its "
                                                "buffer, a hash outside the hash space, or tile records beyond their capacity)", o.tr.overflow ? "tile overflow" : "bucket / key overflow");
    if (!built) {
        if (idx->d_blk_min) drop_blk_min(ctx, idx);
        RK_TRY(alloc_slices(ctx, idx, p));
    }

    RK_TRY(rn.enqueue(false));
    RK_TRY(rn.join());
    BuildResult r = built ? o.r : BuildResult{0, 0, 0, 0, 0};
    if (!built && p.H) {
        RK_TRY(build_general(b, res.p, &r));
        rep[RK_REPORT_GENERAL] = 1;
    } else if (!p.H) RK_TRY(build_empty(b));
    idx->U = r.U;
    idx->n_self = r.n_self;
    idx->slices_refused = p.no_self;
    idx->ref_sets = src.is_set || r.dups == 0;
    idx->built_fast = built;
    if (built) {   // (the same rule as rk_dist.hip plan_self, which counts the records itself for an index built the general way)
        idx->spread = r.flagged * 8 > r.n_self;
        idx->spread_known = 1;
    }
    set_dir_shape(idx);
    guard.p = nullptr;
    *out = idx;
    return RK_OK;
}

}  // namespace

// ---- slice records on first use (an index built with tile records has none) ------------------------------------------
// one thread per posting list: the slice record of every member, by posting position, as the bucket emission writes them
// (class carried by the record: slice_class2).  A list longer than a compact record walks once; the compact ones are short.
__global__ void k_slices_from_lists(const uint32_t *postings, const uint32_t *upos, uint64_t U, uint2 *raw, uint32_t *pos)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const uint32_t s = upos[u], e = upos[u + 1];
    const uint32_t last = e > s ? postings[e - 1] : 0u;
    uint32_t prev = 0xFFFFFFFFu;
    for (uint32_t k = s; k < e; k++) {
        const uint32_t g = postings[k];
        uint2 rec = make_uint2(0, 0);
        if (k + 1 < e) {
            const uint32_t first = postings[k + 1];
            const bool covered = (g & 1u) && prev == g - 1;
            if (last - first <= 31u) {
                uint32_t mask = 0;
                for (uint32_t m = k + 1; m < e; m++) mask |= 1u << (postings[m] - first);
                rec = make_uint2(0x80000000u | first, covered ? mask & ~1u : mask);
            } else {
                rec = make_uint2((k + 1) | (covered ? 0x40000000u : 0u), e | (first - g <= 32u ? 0x80000000u : 0u));
            }
        }
        raw[k] = rec;
        pos[k] = k;
        prev = g;
    }
}
__global__ void k_gather_slices(const uint2 *raw, const uint32_t *sorted_pos, uint64_t H, uint2 *out)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < H) out[e] = raw[sorted_pos[e]];
}

int rk_index_ensure_slices(rk_ctx *ctx, rk_index *idx, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(idx->lazy_mu);
    if (idx->d_selfrange) return RK_OK;
    // (the raw record keeps its class in bit 30 of a posting offset: as in the fast build, H < 2^30 -- every index that was built
    // with tile records is)
    if (idx->slices_refused || idx->H >= (1ULL << 30) || !idx->ref_sets || !idx->d_src_off || idx->wide != (idx->d_uhash64 != nullptr))
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "this index has no slice records (2^31 postings or more, or RK_INDEX_NO_SELF): only sparse self "
                                                "joins (a threshold below distance 1.0) run on it");
    const auto t_begin = std::chrono::steady_clock::now();
    const uint64_t H = idx->H, U = idx->U;
    const uint32_t N = idx->n_ref;
    DevBuf<uint2> raw(ctx), self_raw(ctx), out(ctx);
    DevBuf<uint32_t> pos(ctx), keys_sorted(ctx), pos_sorted(ctx), n_open(ctx), n_cov(ctx);
    DevBuf<uint64_t> self_off(ctx), self_split(ctx);
    DevBuf<BuildResult> res(ctx);
    RK_HIP(ctx, raw.alloc(H));
    RK_HIP(ctx, self_raw.alloc(H));
    RK_HIP(ctx, out.alloc(H + 1));
    RK_HIP(ctx, pos.alloc(H));
    RK_HIP(ctx, keys_sorted.alloc(H));
    RK_HIP(ctx, pos_sorted.alloc(H));
    RK_HIP(ctx, n_open.alloc((size_t)N + 1));
    RK_HIP(ctx, n_cov.alloc((size_t)N + 1));
    RK_HIP(ctx, self_off.alloc((size_t)N + 1));
    RK_HIP(ctx, self_split.alloc((size_t)N + 1));
    RK_HIP(ctx, res.alloc(1));
    RK_HIP(ctx, hipMemsetAsync(res.p, 0, sizeof(BuildResult), st));
    BuildResult r{0, 0, 0, 0, 0};
    if (H) {
        hipLaunchKernelGGL(k_slices_from_lists, dim3(blocks_for(U)), dim3(kThreads), 0, st, idx->d_postings, idx->d_upos, U, raw.p, pos.p);
        RK_HIP(ctx, hipGetLastError());
        // a genome's elements in ascending hash order = its row (the sketches are sets, sorted): a STABLE sort of the posting
        // positions by genome
        int gbits = 1;
        while ((1ULL << gbits) < N) gbits++;
        RK_TRY(rk_prim_sort_pairs_u32_u32(ctx, idx->d_postings, keys_sorted.p, pos.p, pos_sorted.p, H, (unsigned)gbits, st));
        hipLaunchKernelGGL(k_gather_slices, dim3(blocks_for(H)), dim3(kThreads), 0, st, raw.p, pos_sorted.p, H, self_raw.p);
        const unsigned wave_blocks = (N + 3) / 4;
        hipLaunchKernelGGL(k_row_counts2, dim3(wave_blocks), dim3(kThreads), 0, st, idx->d_src_off, N, self_raw.p, n_open.p, n_cov.p);
        hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(1024), 0, st, n_open.p, n_cov.p, N, self_off.p, self_split.p, res.p);
        hipLaunchKernelGGL(k_row_place2, dim3(wave_blocks), dim3(kThreads), 0, st, idx->d_src_off, N, self_raw.p, self_off.p, self_split.p, out.p);
        RK_HIP(ctx, hipGetLastError());
        RK_TRY(rk_read_back(ctx, &r, res.p, sizeof(r), st));
    } else {
        RK_HIP(ctx, hipMemsetAsync(self_off.p, 0, ((size_t)N + 1) * 8, st));
        RK_HIP(ctx, hipMemsetAsync(self_split.p, 0, ((size_t)N + 1) * 8, st));
        RK_HIP(ctx, hipStreamSynchronize(st));
    }
    idx->n_self = r.n_self;
    idx->d_self_off = self_off.release();
    idx->d_self_split = self_split.release();
    idx->d_selfrange = out.release();   // (last: the other threads test this pointer)
    if (ctx->sw_dist_debug)
        fprintf(stderr, "[rk] slice records built on first use: %llu records in %.3f ms\n", (unsigned long long)r.n_self,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    return RK_OK;
}

// prefix directory into the sorted distinct hashes: built on first use (64-bit hashes, hash spaces above 2^30)
int rk_index_ensure_dir(rk_ctx *ctx, rk_index *idx, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(idx->lazy_mu);
    if (idx->d_dir) return RK_OK;
    const uint32_t nb = 1u << idx->dir_bits;
    DevBuf<uint32_t> dir(ctx);
    RK_HIP(ctx, dir.alloc((size_t)nb + 1));
    if (idx->wide)
        hipLaunchKernelGGL(k_dir<uint64_t>, dim3(blocks_for((uint64_t)nb + 1)), dim3(kThreads), 0, st,
                           idx->d_uhash64, idx->U, idx->dir_shift, nb, dir.p);
    else
        hipLaunchKernelGGL(k_dir<uint32_t>, dim3(blocks_for((uint64_t)nb + 1)), dim3(kThreads), 0, st,
                           idx->d_uhash, idx->U, idx->dir_shift, nb, dir.p);
    RK_HIP(ctx, hipGetLastError());
    RK_HIP(ctx, hipStreamSynchronize(st));  // once per index: a later call may come on another stream
    idx->d_dir = dir.release();
    return RK_OK;
}

extern "C" {

void rk_index_free(rk_index *idx)
{
    if (!idx) return;
    rk_ctx *ctx = idx->ctx;
    rk_pool_free(ctx, idx->d_postings);
    rk_pool_free(ctx, idx->d_uhash);
    rk_pool_free(ctx, idx->d_uhash64);
    rk_pool_free(ctx, idx->d_upos);
    rk_pool_free(ctx, idx->d_dir);
    rk_pool_free(ctx, idx->d_rankbm);
    rk_pool_free(ctx, idx->d_rankbase);
    rk_pool_free(ctx, idx->d_urec);
    rk_pool_free(ctx, idx->d_sizes);
    rk_pool_free(ctx, idx->d_selfrange);
    rk_pool_free(ctx, idx->d_shard_rec);
    rk_pool_free(ctx, idx->d_self_off);
    rk_pool_free(ctx, idx->d_self_split);
    rk_pool_free(ctx, idx->d_src_off);
    rk_pool_free(ctx, idx->d_orig);
    rk_pool_free(ctx, idx->d_fb);
    rk_pool_free(ctx, idx->d_tile_contrib);
    rk_pool_free(ctx, idx->d_tile_rows);
    rk_pool_free(ctx, idx->d_tile_cols);
    rk_pool_free(ctx, idx->d_tile_key);
    rk_pool_free(ctx, idx->d_tile_start);
    rk_pool_free(ctx, idx->d_blk_min);
    rk_pool_free(ctx, idx->d_tile_dir[0]);
    rk_pool_free(ctx, idx->d_tile_dir[1]);
    rk_pool_free(ctx, idx->d_tile_order[0]);
    rk_pool_free(ctx, idx->d_tile_order[1]);
    if (idx->h_fb_seen) (void)hipHostFree(idx->h_fb_seen);
    if (idx->fb_event) (void)hipEventDestroy((hipEvent_t)idx->fb_event);
    delete idx;
}

int rk_index_order(const rk_index *idx, uint32_t *orig_out)
{
    if (!idx || (!orig_out && idx->n_ref)) return RK_ERR_ARG;
    rk_ctx *ctx = idx->ctx;
    if (!idx->relabeled || !idx->d_orig) {
        for (uint32_t i = 0; i < idx->n_ref; i++) orig_out[i] = i;
        return RK_OK;
    }
    RK_HIP(ctx, hipSetDevice(ctx->device));
    RK_HIP(ctx, hipMemcpyAsync(orig_out, idx->d_orig, (size_t)idx->n_ref * 4, hipMemcpyDeviceToHost, ctx->stream));
    RK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RK_OK;
}

uint64_t rk_index_total(const rk_index *idx) { return idx ? idx->H : 0; }
uint64_t rk_index_distinct(const rk_index *idx) { return idx ? idx->U : 0; }
uint32_t rk_index_genomes(const rk_index *idx) { return idx ? idx->n_ref : 0; }
int rk_index_hash_bits(const rk_index *idx) { return idx ? idx->hash_bits : 0; }
int rk_index_built_fast(const rk_index *idx) { return idx && idx->built_fast ? 1 : 0; }
int rk_index_build_report(const rk_index *idx, uint64_t out[8])
{
    if (!idx || !out) return RK_ERR_ARG;
    for (int i = 0; i < RK_REPORT_WORDS; i++) out[i] = idx->build_report[i];
    return RK_OK;
}
int rk_index_products(const rk_index *idx)
{
    if (!idx) return 0;
    return (idx->d_selfrange ? 1 : 0) | (idx->tiles_ready ? 2 : 0) | (idx->tiles_ready && idx->tiles_from_build ? 4 : 0);
}

uint64_t rk_index_sum_sq(const rk_index *cidx)
{
    if (!cidx) return 0;
    rk_index *idx = const_cast<rk_index *>(cidx);  // cached on first use: only the roofline report asks for it
    std::lock_guard<std::mutex> lk(idx->lazy_mu);
    if (idx->sum_sq_known) return idx->sum_sq;
    rk_ctx *ctx = idx->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return 0;
    DevBuf<unsigned long long> acc(ctx);
    if (acc.alloc(1) != hipSuccess || hipMemsetAsync(acc.p, 0, 8, ctx->stream) != hipSuccess) return 0;
    if (idx->U)
        hipLaunchKernelGGL(k_sum_sq, dim3(blocks_for(idx->U)), dim3(kThreads), 0, ctx->stream, idx->d_upos, idx->U, acc.p);
    unsigned long long ss = 0;
    if (rk_read_back(ctx, &ss, acc.p, 8, ctx->stream) != RK_OK) return 0;
    idx->sum_sq = ss;
    idx->sum_sq_known = true;
    return ss;
}

int rk_index_self_stats(const rk_index *cidx, uint64_t out[4])
{
    if (!cidx || !out) return RK_ERR_ARG;
    rk_index *idx = const_cast<rk_index *>(cidx);
    std::lock_guard<std::mutex> lk(idx->lazy_mu);
    rk_ctx *ctx = idx->ctx;
    if (!idx->self_stats_known && idx->d_selfrange && idx->n_ref) {
        RK_HIP(ctx, hipSetDevice(ctx->device));
        DevBuf<unsigned long long> acc(ctx);
        RK_HIP(ctx, acc.alloc(2));
        RK_HIP(ctx, hipMemsetAsync(acc.p, 0, 16, ctx->stream));
        hipLaunchKernelGGL(k_self_stats, dim3((idx->n_ref + 3) / 4), dim3(kThreads), 0, ctx->stream, idx->d_selfrange, idx->d_self_off,
                           idx->d_self_split, idx->n_ref, acc.p);
        RK_HIP(ctx, hipGetLastError());
        unsigned long long v[2] = {0, 0};
        RK_TRY(rk_read_back(ctx, v, acc.p, 16, ctx->stream));
        idx->self_stats[0] = idx->n_self;
        idx->self_stats[1] = v[0];
        idx->self_stats[2] = v[1];
        idx->self_stats_known = true;
    }
    idx->self_stats[3] = idx->tiles_ready ? idx->n_tile_records : 0;
    for (int i = 0; i < 4; i++) out[i] = idx->self_stats[i];
    return RK_OK;
}


// (a failing build may leave kernels in flight on both of the context's streams that still write into temporaries its DevBufs
// have just returned to the pool: nothing may be handed out again before they are done)
static int settle_streams(rk_ctx *ctx, int rc)
{
    if (rc && ctx) {
        if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
    }
    return rc;
}

int rk_index_build(rk_ctx *ctx, const rk_sketches *s, int hash_bits, rk_index **out)
{
    if (!ctx || !s || !out) return RK_ERR_ARG;
    return settle_streams(ctx, index_build_impl(ctx, source_of(s), hash_bits, 0, 1, out));
}

int rk_index_build_plan(rk_ctx *ctx, const rk_sketches *s, int hash_bits, uint32_t shard, uint32_t n_shards, int64_t out[])
{
    if (!ctx) return RK_ERR_ARG;
    if (!n_shards || n_shards > kRecRegions || (n_shards & (n_shards - 1)) || shard >= n_shards)
        return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_plan: %u shards (a power of two up to %u), shard %u", n_shards, kRecRegions, shard);
    if (!s || !out) return RK_ERR_ARG;
    // exactly what index_build_impl decides before its first launch: the knobs, the plan, the first attempt's plan
    const BuildKnobs k = read_knobs();
    BuildPlan p;
    RK_TRY(plan_build(ctx, source_of(s), hash_bits, shard, n_shards, k, &p));
    AttemptPlan a;
    RK_TRY(plan_attempt(ctx, p, k, RetryState{p.tiles_mode}, &a));
    out[RK_PLAN_FAST_OK] = p.fast_ok();
    out[RK_PLAN_TILES_MODE] = p.tiles_mode;
    out[RK_PLAN_SLICES_OK] = p.slices_ok;
    out[RK_PLAN_TILES_OK] = p.tiles_ok;
    out[RK_PLAN_B] = p.B;
    out[RK_PLAN_LOW_BITS] = p.low_bits;
    out[RK_PLAN_GB] = p.gb;
    out[RK_PLAN_RB] = p.rb;
    out[RK_PLAN_N_PASS] = p.n_pass;
    out[RK_PLAN_RANGE_BITS] = p.range_bits;
    out[RK_PLAN_PART2] = a.part2;
    out[RK_PLAN_USE_FILTER] = a.use_filter;
    out[RK_PLAN_SMALL_WGS] = a.small_wgs;
    out[RK_PLAN_NARROW] = a.narrow;
    out[RK_PLAN_BIG_OK] = a.big_ok;
    out[RK_PLAN_RELABEL] = p.relabel;
    out[RK_PLAN_TWO_STREAMS] = p.two_streams;
    out[RK_PLAN_EMIT_T] = with_emit_shape(k.emit_t, a.narrow, [](auto threads, auto) -> int { return decltype(threads)::value; });
    out[RK_PLAN_KEYS_CAP] = (int64_t)a.keys_cap;
    out[RK_PLAN_REC_CAP] = (int64_t)a.rec_cap;
    return RK_OK;
}

int rk_index_build_shard(rk_ctx *ctx, const rk_sketches *s, int hash_bits, uint32_t shard, uint32_t n_shards, rk_index **out)
{
    if (!ctx) return RK_ERR_ARG;
    if (!n_shards || n_shards > kRecRegions || (n_shards & (n_shards - 1)) || shard >= n_shards)
        return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_shard: %u shards (a power of two up to %u), shard %u", n_shards, kRecRegions, shard);
    if (!s || !out) return RK_ERR_ARG;
    return settle_streams(ctx, index_build_impl(ctx, source_of(s), hash_bits, shard, n_shards, out));
}


// ---- the exchange of a sharded build -----------------------------------------------------------------------------
namespace {
struct PackArgs {
    unsigned long long dst[kRecRegions];   // where region q's records go in the send buffer
    unsigned long long cnt[kRecRegions];
};
// one workgroup row per region: its valid records to their place in the send buffer (contiguous by destination shard)
__global__ void k_shard_pack(const uint3 *rec, uint32_t region_cap, PackArgs pa, uint3 *out)
{
    const uint32_t q = blockIdx.y;
    const unsigned long long n = pa.cnt[q];
    const uint3 *src = rec + (size_t)q * region_cap;
    uint3 *dst = out + pa.dst[q];
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) dst[i] = src[i];
}
// the received records as kRecRegions equal virtual regions for the tile sort: region q holds records [q * cap, min(n, (q + 1) * cap))
__global__ void k_virtual_regions(unsigned long long n, uint32_t cap, unsigned long long *rec_count)
{
    const uint32_t q = threadIdx.x;
    if (q >= kRecRegions) return;
    const unsigned long long lo = (unsigned long long)q * cap;
    rec_count[q] = n > lo ? min((unsigned long long)cap, n - lo) : 0ULL;
}
}  // namespace

int rk_index_shard_records(const rk_index *idx, uint64_t *counts_out)
{
    if (!idx || !counts_out) return RK_ERR_ARG;
    if (!idx->d_shard_rec || !idx->n_shards) return rk_fail(idx->ctx, RK_ERR_ARG, "not a shard of a sharded build (rk_index_build_shard)");
    const uint32_t sub = kRecRegions / idx->n_shards;
    for (uint32_t d = 0; d < idx->n_shards; d++) {
        counts_out[d] = 0;
        for (uint32_t q = d * sub; q < (d + 1) * sub; q++) counts_out[d] += idx->shard_rec_count[q];
    }
    return RK_OK;
}

int rk_index_shard_pack(const rk_index *idx, void *send_dev, void *stream_v)
{
    if (!idx || !send_dev) return RK_ERR_ARG;
    rk_ctx *ctx = idx->ctx;
    if (!idx->d_shard_rec || !idx->n_shards) return rk_fail(ctx, RK_ERR_ARG, "not a shard of a sharded build (rk_index_build_shard)");
    RK_HIP(ctx, hipSetDevice(ctx->device));
    PackArgs pa;
    unsigned long long at = 0;
    for (uint32_t q = 0; q < kRecRegions; q++) {   // (regions are numbered destination-major)
        pa.dst[q] = at;
        pa.cnt[q] = idx->shard_rec_count[q];
        at += pa.cnt[q];
    }
    if (at) hipLaunchKernelGGL(k_shard_pack, dim3(64, kRecRegions), dim3(256), 0, (hipStream_t)stream_v, idx->d_shard_rec, idx->shard_region_cap, pa, (uint3 *)send_dev);
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}

// ---- a sharded build from per-rank sketches (rk_index_keys.inc) ---------------------------------------------------------
static int checked_shard_bits(rk_ctx *ctx, const char *fn, uint32_t n_shards, int *bits)
{
    if (!n_shards || n_shards > kRecRegions || (n_shards & (n_shards - 1)))
        return rk_fail(ctx, RK_ERR_ARG, "%s: %u shards (a power of two up to %u)", fn, n_shards, kRecRegions);
    *bits = shard_bits_of(n_shards);
    return RK_OK;
}

// the checks both halves of the split share; fills the kernel arguments
static int split_args(rk_ctx *ctx, const char *fn, const rk_sketches *local, uint32_t genome_base, uint32_t n_genomes, int hash_bits,
                      uint32_t n_shards, SplitArgs *a)
{
    int shard_bits = 0;
    RK_TRY(checked_shard_bits(ctx, fn, n_shards, &shard_bits));
    if (!local->n || (uint64_t)genome_base + local->n > n_genomes)
        return rk_fail(ctx, RK_ERR_ARG, "%s: genomes %u .. %llu of a collection of %u", fn, genome_base, (unsigned long long)genome_base + local->n, n_genomes);
    if (hash_bits < 1 || hash_bits > 64 || (hash_bits > 32) != local->wide || hash_bits <= shard_bits)
        return rk_fail(ctx, RK_ERR_ARG, "%s: hash_bits=%d with %s-bit sketches and %u shards", fn, hash_bits, local->wide ? "64" : "32", n_shards);
    if (!local->is_set)
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: a sharded build needs set sketches (a genome lists a hash twice)", fn);
    const int gb = genome_bits_of(n_genomes);
    if (hash_bits - shard_bits + gb > 64)
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: a key of %d hash bits and %d genome bits does not fit 64 bits", fn, hash_bits - shard_bits, gb);
    a->hashes = local->wide ? (const void *)local->d_hashes64 : (const void *)local->d_hashes;
    a->off = local->d_off;
    a->H = local->total;
    a->n_local = local->n;
    a->genome_base = genome_base;
    a->hash_bits = hash_bits;
    a->shift = hash_bits - shard_bits;
    a->gb = gb;
    a->rem_mask = a->shift >= 64 ? ~0ULL : (1ULL << a->shift) - 1ULL;
    a->n_dest = n_shards;
    a->xcd_map = read_knobs().xcd_map;
    return RK_OK;
}

int rk_sketches_signature(rk_ctx *ctx, const rk_sketches *local, void *sig_dev, void *stream)
{
    if (!ctx || !local || !sig_dev) return RK_ERR_ARG;
    if (local->max_size > 0xFFFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_sketches_signature: a sketch of 2^32 hashes or more");
    RK_HIP(ctx, hipSetDevice(ctx->device));
    if (!local->n) return RK_OK;
    const hipStream_t st = (hipStream_t)stream;
    if (local->wide)
        hipLaunchKernelGGL(k_sketch_signature<uint64_t>, dim3(blocks_for(local->n)), dim3(kThreads), 0, st, local->d_hashes64, local->d_off, local->n, (uint32_t *)sig_dev);
    else
        hipLaunchKernelGGL(k_sketch_signature<uint32_t>, dim3(blocks_for(local->n)), dim3(kThreads), 0, st, local->d_hashes, local->d_off, local->n, (uint32_t *)sig_dev);
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}

int rk_sketches_shard_keys(rk_ctx *ctx, const rk_sketches *local, uint32_t genome_base, uint32_t n_genomes, int hash_bits, uint32_t n_shards,
                           uint64_t *counts_out)
{
    if (!ctx || !local || !counts_out) return RK_ERR_ARG;
    SplitArgs a;
    RK_TRY(split_args(ctx, "rk_sketches_shard_keys", local, genome_base, n_genomes, hash_bits, n_shards, &a));
    RK_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    DevBuf<unsigned long long> cnt(ctx);   // [0, 64) keys per destination, [64] the outside-the-hash-space flag
    RK_HIP(ctx, cnt.alloc(kRecRegions + 1));
    RK_HIP(ctx, hipMemsetAsync(cnt.p, 0, (kRecRegions + 1) * 8, st));
    const uint32_t n_chunks = (uint32_t)((a.H + kPartChunk - 1) / kPartChunk);
    unsigned int *bad = reinterpret_cast<unsigned int *>(cnt.p + kRecRegions);
    if (n_chunks) {
        if (local->wide) hipLaunchKernelGGL((k_sketch_split<uint64_t, false>), dim3(n_chunks * kSplitPerChunk), dim3(kSplitThreads), 0, st, a, nullptr, cnt.p, nullptr, bad);
        else hipLaunchKernelGGL((k_sketch_split<uint32_t, false>), dim3(n_chunks * kSplitPerChunk), dim3(kSplitThreads), 0, st, a, nullptr, cnt.p, nullptr, bad);
        RK_HIP(ctx, hipGetLastError());
    }
    unsigned long long v[kRecRegions + 1];
    RK_TRY(rk_read_back(ctx, v, cnt.p, sizeof v, st));
    if (v[kRecRegions])
        return rk_fail(ctx, RK_ERR_ARG, "rk_sketches_shard_keys: a hash beyond %d bits", hash_bits);
    for (uint32_t d = 0; d < n_shards; d++) counts_out[d] = v[d];
    return RK_OK;
}

int rk_sketches_shard_pack(rk_ctx *ctx, const rk_sketches *local, uint32_t genome_base, uint32_t n_genomes, int hash_bits, uint32_t n_shards,
                           void *send_dev, void *stream)
{
    if (!ctx || !local || !send_dev) return RK_ERR_ARG;
    SplitArgs a;
    RK_TRY(split_args(ctx, "rk_sketches_shard_pack", local, genome_base, n_genomes, hash_bits, n_shards, &a));
    RK_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n_chunks = (uint32_t)((a.H + kPartChunk - 1) / kPartChunk);
    if (!n_chunks) return RK_OK;
    const hipStream_t st = (hipStream_t)stream;
    // (the temporaries go back to the pool once the stream has passed the kernels that use them: the call does not wait)
    // [0, 64) keys per destination, [64, 128) cursors into the send buffer, [128] the count pass's flag for hashes beyond hash_bits
    // (rk_sketches_shard_keys reports them; the pack leaves them out)
    DevBuf<unsigned long long> cnt(ctx);
    DevBuf<uint32_t> chunk_first(ctx);
    RK_HIP(ctx, cnt.alloc(2 * kRecRegions + 1));
    RK_HIP(ctx, chunk_first.alloc((size_t)n_chunks + 1));
    hipLaunchKernelGGL(k_chunk_first, dim3(blocks_for(std::max<uint64_t>((uint64_t)n_chunks + 1, 2 * kRecRegions))), dim3(kThreads), 0, st, a.off, a.n_local,
                       n_chunks, chunk_first.p, cnt.p, 2 * kRecRegions + 1);
    unsigned int *const bad = reinterpret_cast<unsigned int *>(cnt.p + 2 * kRecRegions);
    const dim3 grid(n_chunks * kSplitPerChunk);
    if (local->wide) {
        hipLaunchKernelGGL((k_sketch_split<uint64_t, false>), grid, dim3(kSplitThreads), 0, st, a, nullptr, cnt.p, nullptr, bad);
        hipLaunchKernelGGL(k_split_bases, dim3(1), dim3(64), 0, st, cnt.p, n_shards, cnt.p + kRecRegions);
        hipLaunchKernelGGL((k_sketch_split<uint64_t, true>), grid, dim3(kSplitThreads), 0, st, a, chunk_first.p, cnt.p + kRecRegions, (unsigned long long *)send_dev, nullptr);
    } else {
        hipLaunchKernelGGL((k_sketch_split<uint32_t, false>), grid, dim3(kSplitThreads), 0, st, a, nullptr, cnt.p, nullptr, bad);
        hipLaunchKernelGGL(k_split_bases, dim3(1), dim3(64), 0, st, cnt.p, n_shards, cnt.p + kRecRegions);
        hipLaunchKernelGGL((k_sketch_split<uint32_t, true>), grid, dim3(kSplitThreads), 0, st, a, chunk_first.p, cnt.p + kRecRegions, (unsigned long long *)send_dev, nullptr);
    }
    RK_HIP(ctx, hipGetLastError());
    rk_pool_free_after(ctx, cnt.release(), st);
    rk_pool_free_after(ctx, chunk_first.release(), st);
    return RK_OK;
}

int rk_index_build_shard_keys(rk_ctx *ctx, const void *keys_dev, uint64_t n_keys, const void *sig_dev, uint32_t n_genomes, int hash_bits, uint32_t shard,
                              uint32_t n_shards, rk_index **out)
{
    if (!ctx || !out || !sig_dev || (!keys_dev && n_keys)) return RK_ERR_ARG;
    *out = nullptr;
    int shard_bits = 0;
    RK_TRY(checked_shard_bits(ctx, "rk_index_build_shard_keys", n_shards, &shard_bits));
    if (n_shards < 2 || shard >= n_shards)
        return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_shard_keys: shard %u of %u (2 .. %u shards; one is rk_index_build)", shard, n_shards, kRecRegions);
    if (!n_genomes || n_genomes >= 0x7FFFFFFFu) return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_shard_keys: %u genomes", n_genomes);
    if (hash_bits < 1 || hash_bits > 64 || hash_bits <= shard_bits) return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_shard_keys: hash_bits=%d, %u shards", hash_bits, n_shards);
    if (hash_bits - shard_bits + genome_bits_of(n_genomes) > 64)
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_index_build_shard_keys: a key of %d hash bits and %d genome bits does not fit 64 bits", hash_bits - shard_bits,
                       genome_bits_of(n_genomes));
    RK_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const uint32_t N = n_genomes;
    const uint32_t *sig = static_cast<const uint32_t *>(sig_dev);
    // the genomes as the build reads them: their sizes (caller's order) and the signatures themselves (the renumbering reads the first
    // min(size, 16) hashes of every genome from them: the values rk_index_build_shard's renumbering reads of the sketches)
    DevBuf<uint32_t> sizes(ctx);
    DevBuf<unsigned long long> stats(ctx);
    RK_HIP(ctx, sizes.alloc(N));
    RK_HIP(ctx, stats.alloc(3));
    RK_HIP(ctx, hipMemsetAsync(stats.p, 0, 16, st));
    RK_HIP(ctx, hipMemsetAsync(stats.p + 2, 0xFF, 8, st));
    hipLaunchKernelGGL(k_sig_sizes, dim3(std::min<uint32_t>(kSigSizesBlocks, (N + kSigSizesThreads - 1) / kSigSizesThreads)), dim3(kSigSizesThreads), 0, st,
                       sig, N, sizes.p, stats.p);
    RK_HIP(ctx, hipGetLastError());
    unsigned long long st3[3];
    RK_TRY(rk_read_back(ctx, st3, stats.p, sizeof st3, st));
    if (n_keys > st3[0])
        return rk_fail(ctx, RK_ERR_ARG, "rk_index_build_shard_keys: %llu keys, but the signatures count %llu postings", (unsigned long long)n_keys, st3[0]);
    BuildSource src;
    src.n = N;
    src.total = st3[0];
    src.wide = hash_bits > 32;
    src.is_set = true;   // (rk_sketches_shard_pack refuses sketches that are not sets)
    src.max_size = st3[1];
    src.min_size = st3[2] == 0xFFFFFFFFULL ? 0 : st3[2];
    src.d_sizes = sizes.p;
    src.d_sig = sig;
    src.keys = static_cast<const unsigned long long *>(keys_dev);
    src.n_keys = n_keys;
    return settle_streams(ctx, index_build_impl(ctx, src, hash_bits, shard, n_shards, out));
}

// One process, one context per GPU (what `rabbit_kssd alldist --gpus N` does): the all-to-all of the shards' tile records by
// direct copies -- GPU d pulls chunk d of every shard's packed records over its own links (hipMemcpyPeerAsync; on one device a
// plain copy), no communicator.  recv_dev[d] (library-owned: rk_dev_free on parts[d]'s context) holds what shard d joins.
int rk_index_shard_exchange(rk_index *const *parts, uint32_t n, void **recv_dev, uint64_t *n_recv)
{
    if (!parts || !n || !recv_dev || !n_recv || n > kRecRegions) return RK_ERR_ARG;
    for (uint32_t r = 0; r < n; r++) {
        recv_dev[r] = nullptr;
        n_recv[r] = 0;
        if (!parts[r] || !parts[r]->d_shard_rec || parts[r]->n_shards != n || parts[r]->shard_id != r)
            return rk_fail(parts[0] ? parts[0]->ctx : nullptr, RK_ERR_ARG, "rk_index_shard_exchange: parts[r] must be shard r of %u (rk_index_build_shard)", n);
    }
    std::vector<std::vector<uint64_t>> cnt(n, std::vector<uint64_t>(n, 0));
    std::vector<uint3 *> send(n, nullptr);
    auto cleanup = [&](bool also_recv) {
        for (uint32_t r = 0; r < n; r++) {
            rk_ctx *c = parts[r]->ctx;
            if (hipSetDevice(c->device) == hipSuccess) (void)hipStreamSynchronize(c->stream);
            if (send[r]) rk_pool_free(c, send[r]);
            if (also_recv && recv_dev[r]) { (void)hipFree(recv_dev[r]); recv_dev[r] = nullptr; }   // (plain hipMalloc: the caller frees with rk_dev_free)
        }
        (void)hipGetLastError();
    };
    for (uint32_t r = 0; r < n; r++) {   // every shard packs its records, contiguous by destination
        rk_ctx *c = parts[r]->ctx;
        int rc = rk_index_shard_records(parts[r], cnt[r].data());
        if (rc) { cleanup(true); return rc; }
        uint64_t tot = 0;
        for (uint32_t d = 0; d < n; d++) tot += cnt[r][d];
        if (hipSetDevice(c->device) != hipSuccess) { cleanup(true); return rk_fail(c, RK_ERR_HIP, "cannot select device %d", c->device); }
        send[r] = static_cast<uint3 *>(rk_pool_alloc(c, std::max<uint64_t>(1, tot) * sizeof(uint3)));
        if (!send[r]) { cleanup(true); return rk_fail(c, RK_ERR_NOMEM, "cannot allocate the send buffer of %llu tile records", (unsigned long long)tot); }
        rc = rk_index_shard_pack(parts[r], send[r], c->stream);
        if (rc) { cleanup(true); return rc; }
    }
    for (uint32_t r = 0; r < n; r++) {
        rk_ctx *c = parts[r]->ctx;
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { cleanup(true); return rk_fail(c, RK_ERR_HIP, "packing the tile records of shard %u failed", r); }
    }
    for (uint32_t d = 0; d < n; d++) {   // every destination pulls its chunks
        rk_ctx *c = parts[d]->ctx;
        uint64_t tot = 0;
        for (uint32_t r = 0; r < n; r++) tot += cnt[r][d];
        n_recv[d] = tot;
        if (hipSetDevice(c->device) != hipSuccess) { cleanup(true); return rk_fail(c, RK_ERR_HIP, "cannot select device %d", c->device); }
        if (hipMalloc(&recv_dev[d], std::max<uint64_t>(1, tot) * sizeof(uint3)) != hipSuccess) {
            recv_dev[d] = nullptr;
            (void)hipGetLastError();
            cleanup(true);
            return rk_fail(c, RK_ERR_NOMEM, "cannot allocate the receive buffer of %llu tile records", (unsigned long long)tot);
        }
        uint64_t at = 0;
        for (uint32_t r = 0; r < n; r++) {
            const uint64_t c_rd = cnt[r][d];
            if (!c_rd) continue;
            uint64_t from = 0;
            for (uint32_t q = 0; q < d; q++) from += cnt[r][q];
            rk_ctx *sc = parts[r]->ctx;
            uint3 *dst = static_cast<uint3 *>(recv_dev[d]) + at;
            hipError_t e;
            if (sc->device == c->device) e = hipMemcpyAsync(dst, send[r] + from, c_rd * sizeof(uint3), hipMemcpyDeviceToDevice, c->stream);
            else {
                int can = 0;
                (void)hipDeviceCanAccessPeer(&can, c->device, sc->device);
                if (can && hipDeviceEnablePeerAccess(sc->device, 0) != hipSuccess) (void)hipGetLastError();   // (already enabled)
                e = hipMemcpyPeerAsync(dst, c->device, send[r] + from, sc->device, c_rd * sizeof(uint3), c->stream);
            }
            if (e != hipSuccess) { cleanup(true); return rk_fail(c, RK_ERR_HIP, "copy of tile records from device %d to device %d failed: %s", sc->device, c->device, hipGetErrorString(e)); }
            at += c_rd;
        }
    }
    for (uint32_t d = 0; d < n; d++) {   // bounded wait: a peer copy that never completes must end in an error, not in a hang
        rk_ctx *c = parts[d]->ctx;
        hipError_t qe = hipSetDevice(c->device);
        const auto t_start = std::chrono::steady_clock::now();
        while (qe == hipSuccess) {
            qe = hipStreamQuery(c->stream);
            if (qe != hipErrorNotReady) break;
            if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(120)) break;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
            qe = hipSuccess;
        }
        (void)hipGetLastError();
        if (qe != hipSuccess) {
            // (a copy that is stuck: its buffers are leaked rather than waited for)
            return rk_fail(c, RK_ERR_HIP, "the exchange of tile records did not complete on device %d: %s", c->device, hipGetErrorString(qe));
        }
    }
    for (uint32_t r = 0; r < n; r++) { rk_pool_free(parts[r]->ctx, send[r]); send[r] = nullptr; }
    return RK_OK;
}

int rk_index_join_shard(rk_ctx *ctx, const rk_index *part, const void *recv_dev, uint64_t n_records, rk_index **out)
{
    if (!ctx || !part || !out || (!recv_dev && n_records)) return RK_ERR_ARG;
    *out = nullptr;
    if (!part->d_src_off || !part->d_sizes || !part->n_ref || part->ctx != ctx)
        return rk_fail(ctx, RK_ERR_ARG, "rk_index_join_shard needs an index built on this context (rk_index_build_shard) for the genomes' sizes and order");
    if (n_records >= 0x7FFF0000ULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "more than 2^31 tile records for one shard");
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t N = part->n_ref, n_blocks = (N + 31) / 32;
    if (n_blocks > kTileMaxBlocks) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "more than %u genomes", kTileMaxBlocks * 32);
    rk_index *idx = new (std::nothrow) rk_index;
    if (!idx) return RK_ERR_NOMEM;
    IndexGuard guard{idx};
    idx->ctx = ctx;
    idx->n_ref = N;
    idx->hash_bits = part->hash_bits;
    idx->wide = part->wide;
    idx->ref_sets = true;
    idx->max_src_size = part->max_src_size;
    idx->max_ref_size = part->max_ref_size;
    idx->min_ref_size = part->min_ref_size;
    idx->slices_refused = true;   // (a join-only index: tile records of this shard's rows, no postings)
    RK_TRY(pool_array(ctx, &idx->d_sizes, (size_t)N + 1));
    RK_TRY(pool_array(ctx, &idx->d_src_off, (size_t)N + 1));
    RK_TRY(pool_array(ctx, &idx->d_blk_min, (size_t)n_blocks));
    RK_HIP(ctx, hipMemcpyAsync(idx->d_sizes, part->d_sizes, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    RK_HIP(ctx, hipMemcpyAsync(idx->d_src_off, part->d_src_off, ((size_t)N + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (part->relabeled && part->d_orig) {
        RK_TRY(pool_array(ctx, &idx->d_orig, (size_t)N + 1));
        RK_HIP(ctx, hipMemcpyAsync(idx->d_orig, part->d_orig, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
        idx->relabeled = true;
    }
    hipLaunchKernelGGL(k_blk_min_sizes, dim3(blocks_for(n_blocks)), dim3(kThreads), 0, st, idx->d_sizes, N, n_blocks, idx->d_blk_min);
    const uint32_t region_cap = (uint32_t)std::max<uint64_t>(1, (n_records + kRecRegions - 1) / kRecRegions);
    TileSortBufs sort(ctx);
    RK_TRY(sort.alloc(ctx, n_blocks, n_records, std::max<uint64_t>(1, std::min<uint64_t>(n_records, (uint64_t)n_blocks * (n_blocks + 1) / 2))));
    DevBuf<unsigned long long> zeroed(ctx);
    ZeroedLayout z = ZeroedLayout::of_join(n_blocks);
    RK_HIP(ctx, zeroed.alloc(z.z_end));
    RK_HIP(ctx, hipMemsetAsync(zeroed.p, 0, z.z_end * 8, st));
    z.base = zeroed.p;
    TileResult *const tres = z.tile_res();
    hipLaunchKernelGGL(k_virtual_regions, dim3(1), dim3(64), 0, st, (unsigned long long)n_records, region_cap, &tres->rec_count[0]);
    const TileSortArgs ta = sort.args((const uint3 *)recv_dev, region_cap, n_blocks, idx->d_blk_min, z);
    RK_TRY(launch_tile_sort(ctx, ta, st, []() { return RK_OK; }));
    TileResult tr;
    RK_TRY(rk_read_back(ctx, &tr, tres, sizeof(tr), st));
    if (ctx->sw_dist_debug) {   // (developer output: how the records spread over the row blocks)
        std::vector<uint32_t> bc(n_blocks);
        RK_TRY(rk_read_back(ctx, bc.data(), ta.bin_count, (size_t)n_blocks * 4, st));
        std::sort(bc.begin(), bc.end(), std::greater<uint32_t>());
        unsigned long long top = 0, all = 0;
        uint32_t non_empty = 0;
        for (uint32_t i = 0; i < n_blocks; i++) {
            all += bc[i];
            if (i < 64) top += bc[i];
            non_empty += bc[i] != 0;
        }
        fprintf(stderr, "[rk] join shard: %llu records in %u of %u row blocks; fullest %u, 64th %u, the 64 fullest hold %llu\n", all, non_empty, n_blocks, bc[0],
                bc[std::min<uint32_t>(63, n_blocks - 1)], top);
    }
    sort.hand_over(idx, tr);
    guard.p = nullptr;
    *out = idx;
    return RK_OK;
}

}  // extern "C"
