// rk_mask.hip -- query sketches filtered by an index (rk_sketches_mask), and the same rule on the host over exported lists (rk_mask_lists).
// For a query hash h, c(h) = the length of h's posting list (0 without one; a hash at or beyond 2^hash_bits has none); h survives iff
// min_refs <= c(h) <= max_refs.  {0, 0} is the reference's `sub`, {1, UINT32_MAX} the intersection.  The result has the sketches of the
// queries, in their order, each with its survivors in its own order (a device-resident sketch ascends).  include/rabbitkssd.h,
// filtering query sketches by an index.
//
//   flag      k_mask_flag: flat over ALL query hashes in tiles of kTileHashes, whatever sketch they belong to (sketch sizes range from
//             nothing to millions: a split by sketch would not balance).  A workgroup of kMaskThreads takes a tile, a wave kTrips
//             consecutive runs of 64 hashes: lane l of run t reads element base + 64 t + l (coalesced; the ballot is in element order).
//             The hashes of a lane's kTrips runs are loaded first, then looked up together (index_lookup of rk_query_dev.h: the
//             directory buckets, then the binary searches, one probe of each per step).  Per run one 64-bit keep word, per tile the
//             number of survivors;
//   scan      an exclusive scan of the tile counts in 64 bits (the survivors may pass 2^32, which the 32-bit scan of rk_prims_scan.hip
//             cannot hold): k_mask_scan_tiles, one workgroup per kScanTiles tiles, then k_mask_scan_blocks, one wave over the sums of
//             those workgroups.  tile_prefix() adds the two;
//   scatter   k_mask_scatter: a tile's 32 keep words once per wave (their popcounts scanned across lanes), then every survivor to
//             tile prefix + survivors before it in the tile.  Order is preserved; no atomics;
//             k_mask_scatter<Hash, true> (rk_sketches_mask_counts): the survivor's count goes to the same place of the result's counts;
//   offsets   k_mask_offsets: one lane per offset entry, off_out[g] = the survivors before element off_in[g], from the tile prefix and
//             the keep words of one tile.  No segmented scan; empty sketches fall out by themselves.
//
// Memory scope: every array is written by one kernel and read by a later one on the same stream.  INSIDE a launch the only communication
// between workgroups is relaxed agent-scope adds on three counters nobody reads before the launch is over.  No loop waits for another
// workgroup: any grid works.  The host synchronises once, for the n + 1 offsets and the counters.  DESIGN.md 4.16.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "rk_internal.h"
#include "rk_query_dev.h"

namespace {

constexpr int kMaskThreads = 256;                          // threads of every workgroup of this unit: 4 waves
constexpr int kTrips = 8;                                  // runs of 64 hashes one wave takes of a tile
constexpr int kTileHashes = kMaskThreads * kTrips;         // 2048
constexpr int kTileWords = kTileHashes / 64;               // keep words of a tile
constexpr int kScanTiles = kMaskThreads;                   // tiles one workgroup of the scan takes: one per thread
static_assert(kTileWords == 32 && kMaskThreads == 4 * 64, "k_mask_scatter holds the keep words of a tile in the lower half of a wave");
static_assert(sizeof(rk_mask_rule) == 8 && sizeof(rk_mask_stats) == 56, "the layouts of include/rabbitkssd.h");

struct Counters {   // one device block, read back in one copy
    unsigned long long matched;    // query hashes with a posting list
    unsigned long long repeats;    // survivors that equal the element before them, sketch boundaries ignored (only counted for multiset queries)
    unsigned long long across;     // of which the first element of a sketch: no repeat after all
};

struct MaskArgs {
    const void *q_hashes;              // Hash[total]
    const uint64_t *q_off;             // u64[n + 1]
    unsigned long long total, tiles;
    uint32_t n;
    IndexLookup ix;                    // (U == 0: nothing is looked up, every c(h) is 0)
    const uint32_t *upos;              // u32[U + 1]
    uint32_t min_refs, max_refs;
    uint32_t count_repeats;            // the queries are no sets: the result may or may not be
    unsigned long long *keep;          // u64[tiles * kTileWords]
    uint32_t *tile_kept, *tile_local;  // u32[tiles]: survivors of the tile; of the tiles before it in its scan block
    unsigned long long *block_sum, *block_base;   // u64[scan blocks]
    void *out_hashes;                  // Hash[kept]
    uint64_t *off_out;                 // u64[n + 1]
    Counters *cnt;
    const uint32_t *q_counts;          // u32[total]: rk_sketches_mask_counts only
    uint32_t *out_counts;              // u32[kept]
};

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int delta)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, delta), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), delta);
    return ((unsigned long long)hi << 32) | lo;
}

// survivors before tile t
__device__ __forceinline__ unsigned long long tile_prefix(const MaskArgs &a, unsigned long long t)
{
    return a.block_base[t / kScanTiles] + a.tile_local[t];
}

// (8 waves per SIMD: with the look-up in a function of its own the compiler would keep all of a lane's last probes in flight, at twice
// the registers and half the waves -- k_lca_tally, which its LDS table holds to 3 waves anyway, takes that)
template <class Hash> __global__ void __launch_bounds__(kMaskThreads, 8) k_mask_flag(MaskArgs a)
{
    __shared__ uint32_t s_kept[kMaskThreads / 64], s_matched[kMaskThreads / 64], s_repeats[kMaskThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long tile = blockIdx.x;
    const unsigned long long base = tile * kTileHashes + (unsigned long long)wave * (kTrips * 64);
    const Hash *q = (const Hash *)a.q_hashes;
    unsigned long long h[kTrips];
    uint32_t list[kTrips];
    bool in[kTrips], repeat[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const unsigned long long j = base + 64 * t + lane;
        in[t] = j < a.total;
        h[t] = in[t] ? (unsigned long long)q[j] : 0ULL;
        repeat[t] = a.count_repeats && in[t] && j > 0 && (unsigned long long)q[j - 1] == h[t];
    }
    index_lookup<Hash, kTrips>(a.ix, h, in, list);
    uint32_t kept = 0, matched = 0, repeats = 0;   // (uniform per wave)
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const uint32_t c = list[t] != kNoList ? a.upos[list[t] + 1] - a.upos[list[t]] : 0u;
        const bool keep = in[t] && c >= a.min_refs && c <= a.max_refs;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) a.keep[tile * kTileWords + wave * kTrips + t] = m;
        kept += (uint32_t)__popcll(m);
        matched += (uint32_t)__popcll(__ballot(c > 0));
        repeats += (uint32_t)__popcll(__ballot(keep && repeat[t]));
    }
    if (lane == 0) {
        s_kept[wave] = kept;
        s_matched[wave] = matched;
        s_repeats[wave] = repeats;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t k = 0, m = 0, r = 0;
#pragma unroll
        for (int w = 0; w < kMaskThreads / 64; w++) {
            k += s_kept[w];
            m += s_matched[w];
            r += s_repeats[w];
        }
        a.tile_kept[tile] = k;
        if (m) add_u64(&a.cnt->matched, m);
        if (r) add_u64(&a.cnt->repeats, r);
    }
}

// one workgroup per kScanTiles tiles: the survivors of the tiles before each within the workgroup's span, and the span's sum
__global__ void __launch_bounds__(kMaskThreads) k_mask_scan_tiles(MaskArgs a)
{
    __shared__ uint32_t s_wave[kMaskThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long t = (unsigned long long)blockIdx.x * kScanTiles + threadIdx.x;
    const uint32_t v = t < a.tiles ? a.tile_kept[t] : 0u;
    uint32_t incl = v;   // (a span holds at most kScanTiles * kTileHashes = 2^19 survivors)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kMaskThreads / 64; w++) {
        if (w < wave) before += s_wave[w];
        sum += s_wave[w];
    }
    if (t < a.tiles) a.tile_local[t] = before + incl - v;
    if (threadIdx.x == 0) a.block_sum[blockIdx.x] = sum;
}

// one wave: the exclusive scan of the sums of the scan blocks, 64 at a time with a carry
__global__ void __launch_bounds__(64) k_mask_scan_blocks(MaskArgs a, uint32_t n_blocks)
{
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64) {   // (uniform)
        const uint32_t b = b0 + lane;
        const unsigned long long v = b < n_blocks ? a.block_sum[b] : 0ULL;
        unsigned long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = shfl_up_u64(incl, o);
            if (lane >= o) incl += up;
        }
        if (b < n_blocks) a.block_base[b] = carry + incl - v;
        carry += shfl_u64(incl, 63);
    }
}

// COUNTS: a survivor's count goes along (rk_sketches_mask_counts)
template <class Hash, bool COUNTS> __global__ void __launch_bounds__(kMaskThreads) k_mask_scatter(MaskArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long tile = blockIdx.x;
    if (!a.tile_kept[tile]) return;   // (uniform: nothing of this tile survives)
    const Hash *q = (const Hash *)a.q_hashes;
    Hash *out = (Hash *)a.out_hashes;
    // lanes 0..31 hold the tile's keep words; word_before = the survivors of the words before a lane's
    const unsigned long long word = a.keep[tile * kTileWords + (lane & (kTileWords - 1))];
    const uint32_t pop = (uint32_t)__popcll(word);
    uint32_t incl = pop;
#pragma unroll
    for (int o = 1; o < kTileWords; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += up;
    }
    const uint32_t word_before = incl - pop;
    const unsigned long long first = tile_prefix(a, tile);
    const unsigned long long base = tile * kTileHashes + (unsigned long long)wave * (kTrips * 64);
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const int w = wave * kTrips + t;
        const unsigned long long m = shfl_u64(word, w);
        const uint32_t before = (uint32_t)__shfl((int)word_before, w);
        // (a set bit names an element below total: k_mask_flag set it; its place lies below the sum of all tile counts)
        if (m >> lane & 1ULL) {
            const unsigned long long at = first + before + (uint32_t)__popcll(m & lanes_below(lane));
            out[at] = q[base + 64 * t + lane];
            if constexpr (COUNTS) a.out_counts[at] = a.q_counts[base + 64 * t + lane];
        }
    }
}

// off_out[g] = the survivors before element q_off[g], g = 0 .. n
template <class Hash> __global__ void __launch_bounds__(kMaskThreads) k_mask_offsets(MaskArgs a)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * kMaskThreads + threadIdx.x;
    if (g > a.n) return;
    if (!a.tiles) {   // no hash at all
        a.off_out[g] = 0;
        return;
    }
    const unsigned long long p = a.q_off[g];   // (<= total: the offsets of a sketches object)
    unsigned long long tile = p / kTileHashes;
    uint32_t r = (uint32_t)(p % kTileHashes);
    if (tile >= a.tiles) {   // p == total on a tile boundary: everything of the last tile
        tile = a.tiles - 1;
        r = kTileHashes;
    }
    unsigned long long before = tile_prefix(a, tile);
    const unsigned long long *words = a.keep + tile * kTileWords;
    for (uint32_t w = 0; w < r / 64; w++) before += (unsigned long long)__popcll(words[w]);
    if (r % 64) before += (unsigned long long)__popcll(words[r / 64] & lanes_below((int)(r % 64)));
    a.off_out[g] = before;
    if (a.count_repeats && g < a.n && p > 0 && p < a.q_off[g + 1]) {
        // the first element of a non-empty sketch: if it survives and equals the element before it, k_mask_flag counted a repeat that is none
        const Hash *q = (const Hash *)a.q_hashes;
        if ((words[r / 64] >> (r % 64) & 1ULL) && q[p - 1] == q[p]) add_u64(&a.cnt->across, 1ULL);
    }
}

// ---- host: the rule, exactly ------------------------------------------------------------------------------------------------
void fill_geometry(rk_mask_stats *st, uint64_t hashes)
{
    st->hashes = hashes;
    st->tiles = (hashes + kTileHashes - 1) / kTileHashes;
    st->tile_hashes = kTileHashes;
    st->scan_blocks = (uint32_t)((st->tiles + kScanTiles - 1) / kScanTiles);
    st->threads = kMaskThreads;
}

// the survivors of every query in its own order; off[n_query + 1]; counts what rk_mask_stats counts
// (q_counts with kept_counts: the count of every survivor goes along)
template <class Hash>
void mask_lists(const Hash *q, const uint64_t *q_off, uint32_t n_query, const Hash *list_hashes, const uint32_t *counts, uint64_t n_lists,
                const rk_mask_rule *rule, std::vector<Hash> *kept, uint64_t *off, rk_mask_stats *st, const uint32_t *q_counts = nullptr,
                std::vector<uint32_t> *kept_counts = nullptr)
{
    kept->clear();
    off[0] = 0;
    for (uint32_t i = 0; i < n_query; i++) {
        for (uint64_t j = q_off[i]; j < q_off[i + 1]; j++) {
            const Hash *at = std::lower_bound(list_hashes, list_hashes + n_lists, q[j]);
            const uint32_t c = at != list_hashes + n_lists && *at == q[j] ? counts[at - list_hashes] : 0u;
            st->matched += c > 0;
            if (c >= rule->min_refs && c <= rule->max_refs) {
                kept->push_back(q[j]);
                if (kept_counts) kept_counts->push_back(q_counts[j]);
            }
        }
        off[i + 1] = kept->size();
        st->emptied += q_off[i + 1] > q_off[i] && off[i + 1] == off[i];
    }
    st->kept = kept->size();
}

// RK_MASK_DEVICE=0: download + export + the rule on the host + rk_sketches_from_host(64)
// (with_counts: + rk_sketches_download_counts, the result by rk_sketches_from_host_counts)
template <class Hash>
int mask_on_host(rk_ctx *ctx, const rk_sketches *qs, const rk_index *idx, const rk_mask_rule *rule, bool with_counts, rk_mask_stats *st, rk_sketches **out)
{
    std::vector<Hash> q(qs->total), hashes(idx->U), kept;
    std::vector<uint32_t> qc((size_t)(with_counts ? qs->total : 0)), kc;
    if (with_counts) RK_TRY(rk_sketches_download_counts(qs, qc.data()));
    std::vector<uint32_t> postings(idx->H), counts(idx->U);
    std::vector<uint64_t> off((size_t)qs->n + 1);
    if constexpr (sizeof(Hash) == 8) {
        RK_TRY(rk_sketches_download64(qs, q.data(), nullptr));
        if (idx->U) RK_TRY(rk_index_export64(idx, postings.data(), hashes.data(), counts.data()));
    } else {
        RK_TRY(rk_sketches_download(qs, q.data(), nullptr));
        if (idx->U) RK_TRY(rk_index_export_lists(idx, postings.data(), hashes.data(), counts.data()));
    }
    // (a hash at or beyond 2^hash_bits is none of the exported hashes: the index holds none)
    mask_lists(q.data(), qs->h_off.data(), qs->n, hashes.data(), counts.data(), idx->U, rule, &kept, off.data(), st, with_counts ? qc.data() : nullptr,
               with_counts ? &kc : nullptr);
    if (with_counts) return rk_sketches_from_host_counts(ctx, kept.data(), sizeof(Hash) == 8, kc.data(), off.data(), qs->n, out);
    if constexpr (sizeof(Hash) == 8) return rk_sketches_from_host64(ctx, kept.data(), off.data(), qs->n, out);
    else return rk_sketches_from_host(ctx, kept.data(), off.data(), qs->n, out);
}

int mask_on_device(rk_ctx *ctx, const rk_sketches *qs, const rk_index *idx, const rk_mask_rule *rule, bool with_counts, rk_mask_stats *st, rk_sketches **out)
{
    const uint32_t n = qs->n;
    const uint64_t total = qs->total, tiles = st->tiles;
    if (tiles > 0x7FFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_sketches_mask: more than 2^31 tiles of query hashes");
    RK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const TimedSpan span{ctx, RK_MS_MASK};
    if (idx->U) RK_TRY(rk_index_ensure_dir(ctx, const_cast<rk_index *>(idx), stream));
    DevBuf<unsigned long long> keep(ctx), block_sum(ctx), block_base(ctx);
    DevBuf<uint32_t> tile_kept(ctx), tile_local(ctx);
    DevBuf<Counters> cnt(ctx);
    RK_HIP(ctx, keep.alloc(tiles * kTileWords));
    RK_HIP(ctx, tile_kept.alloc(tiles));
    RK_HIP(ctx, tile_local.alloc(tiles));
    RK_HIP(ctx, block_sum.alloc(st->scan_blocks));
    RK_HIP(ctx, block_base.alloc(st->scan_blocks));
    RK_HIP(ctx, cnt.alloc(1));
    RK_HIP(ctx, hipMemsetAsync(cnt.p, 0, sizeof(Counters), stream));

    rk_sketches *s = new (std::nothrow) rk_sketches;
    if (!s) return RK_ERR_NOMEM;
    SketchesGuard guard{s};
    s->ctx = ctx;
    s->n = n;
    s->wide = qs->wide;
    RK_TRY(pool_array(ctx, &s->d_off, (size_t)n + 1));

    MaskArgs a;
    memset(&a, 0, sizeof a);
    a.q_hashes = qs->wide ? (const void *)qs->d_hashes64 : (const void *)qs->d_hashes;
    a.q_off = qs->d_off;
    a.total = total;
    a.tiles = tiles;
    a.n = n;
    a.ix = index_lookup_of(idx);
    a.upos = idx->d_upos;
    a.min_refs = rule->min_refs;
    a.max_refs = rule->max_refs;
    a.count_repeats = qs->is_set ? 0u : 1u;
    a.keep = keep.p;
    a.tile_kept = tile_kept.p;
    a.tile_local = tile_local.p;
    a.block_sum = block_sum.p;
    a.block_base = block_base.p;
    a.off_out = s->d_off;
    a.cnt = cnt.p;

    RK_HIP(ctx, span.begin());
    if (tiles) {
        if (qs->wide) hipLaunchKernelGGL(k_mask_flag<uint64_t>, dim3((unsigned)tiles), dim3(kMaskThreads), 0, stream, a);
        else hipLaunchKernelGGL(k_mask_flag<uint32_t>, dim3((unsigned)tiles), dim3(kMaskThreads), 0, stream, a);
        hipLaunchKernelGGL(k_mask_scan_tiles, dim3(st->scan_blocks), dim3(kMaskThreads), 0, stream, a);
        hipLaunchKernelGGL(k_mask_scan_blocks, dim3(1), dim3(64), 0, stream, a, st->scan_blocks);
        RK_HIP(ctx, hipGetLastError());
    }
    // the survivors are at most the query hashes: the result's array is sized before their number is known (no synchronisation between
    // the scan and the scatter)
    RK_TRY(with_hash_type(qs->wide, [&](auto ht) -> int {
        using Hash = decltype(ht);
        Hash *&hashes = hashes_of(s, ht);
        RK_TRY(pool_array(ctx, &hashes, total + 1));
        a.out_hashes = hashes;
        if (with_counts) {
            RK_TRY(pool_array(ctx, &s->d_counts, total + 1));
            a.q_counts = qs->d_counts;
            a.out_counts = s->d_counts;
        }
        const auto scatter = with_counts ? k_mask_scatter<Hash, true> : k_mask_scatter<Hash, false>;
        if (tiles) hipLaunchKernelGGL(scatter, dim3((unsigned)tiles), dim3(kMaskThreads), 0, stream, a);
        hipLaunchKernelGGL(k_mask_offsets<Hash>, dim3(blocks_for((uint64_t)n + 1, kMaskThreads)), dim3(kMaskThreads), 0, stream, a);
        RK_HIP(ctx, hipGetLastError());
        return RK_OK;
    }));
    RK_HIP(ctx, span.end());
    // the one read-back: the n + 1 offsets and the counters (pageable memory of this function: the stream is synchronised before it returns)
    Counters home;
    s->h_off.assign((size_t)n + 1, 0);
    RK_HIP(ctx, hipMemcpyAsync(s->h_off.data(), s->d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
    RK_HIP(ctx, hipMemcpyAsync(&home, cnt.p, sizeof home, hipMemcpyDeviceToHost, stream));
    RK_HIP(ctx, hipStreamSynchronize(stream));
    span.read();
    if (s->h_off[0] != 0 || s->h_off[n] > total || home.matched > total || home.across > home.repeats)
        return rk_fail(ctx, RK_ERR_HIP, "rk_sketches_mask: more survivors than query hashes (internal error)");
    for (uint32_t g = 0; g < n; g++) {
        if (s->h_off[g + 1] < s->h_off[g] || s->h_off[g + 1] - s->h_off[g] > qs->h_off[g + 1] - qs->h_off[g])
            return rk_fail(ctx, RK_ERR_HIP, "rk_sketches_mask: a sketch with more survivors than hashes (internal error)");
        const uint64_t size = s->h_off[g + 1] - s->h_off[g];
        s->max_size = std::max(s->max_size, size);
        st->emptied += qs->h_off[g + 1] > qs->h_off[g] && !size;
    }
    s->total = s->h_off[n];
    s->is_set = qs->is_set || home.repeats == home.across;   // a subset of a strictly ascending sketch ascends strictly
    st->kept = s->total;
    st->matched = home.matched;
    guard.p = nullptr;
    *out = s;
    return RK_OK;
}

template <class Hash> bool strictly_ascending(const Hash *h, uint64_t n)
{
    for (uint64_t i = 1; i < n; i++)
        if (h[i - 1] >= h[i]) return false;
    return true;
}

// (counts_out with q_counts: rk_mask_lists_counts)
template <class Hash>
int mask_lists_call(const void *q_hashes, const uint64_t *q_off, uint32_t n_query, const void *list_hashes, const uint32_t *counts, uint64_t n_lists,
                    const rk_mask_rule *rule, void **hashes_out, uint64_t *off_out, rk_mask_stats *stats, const uint32_t *q_counts = nullptr,
                    uint32_t **counts_out = nullptr)
{
    if (!strictly_ascending((const Hash *)list_hashes, n_lists)) return RK_ERR_ARG;
    rk_mask_stats st;
    memset(&st, 0, sizeof st);
    fill_geometry(&st, q_off[n_query]);
    st.path = 2;
    std::vector<Hash> kept;
    std::vector<uint64_t> off((size_t)n_query + 1);
    std::vector<uint32_t> kept_counts;
    mask_lists((const Hash *)q_hashes, q_off, n_query, (const Hash *)list_hashes, counts, n_lists, rule, &kept, off.data(), &st, q_counts,
               counts_out ? &kept_counts : nullptr);
    void *h = nullptr;
    uint32_t *c = nullptr;
    if (!kept.empty()) {
        h = malloc(kept.size() * sizeof(Hash));
        if (!h) return RK_ERR_NOMEM;
        memcpy(h, kept.data(), kept.size() * sizeof(Hash));
        if (counts_out) {
            c = (uint32_t *)malloc(kept.size() * 4);
            if (!c) {
                free(h);
                return RK_ERR_NOMEM;
            }
            memcpy(c, kept_counts.data(), kept.size() * 4);
        }
    }
    memcpy(off_out, off.data(), off.size() * 8);
    *hashes_out = h;
    if (counts_out) *counts_out = c;
    if (stats) *stats = st;
    return RK_OK;
}

}  // namespace

extern "C" {

// rk_mask_lists (counts_out == null) and rk_mask_lists_counts
static int mask_lists_entry(const void *q_hashes, const uint32_t *q_counts, int wide, const uint64_t *q_off, uint32_t n_query, const void *list_hashes,
                            const uint32_t *counts, uint64_t n_lists, const rk_mask_rule *rule, void **hashes_out, uint32_t **counts_out, uint64_t *off_out,
                            rk_mask_stats *stats)
{
    if (!q_off || !rule || !hashes_out || !off_out) return RK_ERR_ARG;
    if (rule->min_refs > rule->max_refs) return RK_ERR_ARG;
    if (n_lists && (!list_hashes || !counts)) return RK_ERR_ARG;
    if (q_off[0] != 0) return RK_ERR_ARG;
    for (uint32_t i = 0; i < n_query; i++)
        if (q_off[i + 1] < q_off[i]) return RK_ERR_ARG;
    if (q_off[n_query] && (!q_hashes || (counts_out && !q_counts))) return RK_ERR_ARG;
    return wide ? mask_lists_call<uint64_t>(q_hashes, q_off, n_query, list_hashes, counts, n_lists, rule, hashes_out, off_out, stats, q_counts, counts_out)
                : mask_lists_call<uint32_t>(q_hashes, q_off, n_query, list_hashes, counts, n_lists, rule, hashes_out, off_out, stats, q_counts, counts_out);
}

int rk_mask_lists(const void *q_hashes, int wide, const uint64_t *q_off, uint32_t n_query, const void *list_hashes, const uint32_t *counts, uint64_t n_lists,
                  const rk_mask_rule *rule, void **hashes_out, uint64_t *off_out, rk_mask_stats *stats)
{
    return mask_lists_entry(q_hashes, nullptr, wide, q_off, n_query, list_hashes, counts, n_lists, rule, hashes_out, nullptr, off_out, stats);
}

int rk_mask_lists_counts(const void *q_hashes, const uint32_t *q_counts, int wide, const uint64_t *q_off, uint32_t n_query, const void *list_hashes,
                         const uint32_t *counts, uint64_t n_lists, const rk_mask_rule *rule, void **hashes_out, uint32_t **counts_out, uint64_t *off_out,
                         rk_mask_stats *stats)
{
    if (!counts_out) return RK_ERR_ARG;
    return mask_lists_entry(q_hashes, q_counts, wide, q_off, n_query, list_hashes, counts, n_lists, rule, hashes_out, counts_out, off_out, stats);
}

static int sketches_mask(rk_ctx *ctx, const rk_sketches *queries, const rk_index *idx, const rk_mask_rule *rule, bool with_counts, rk_sketches **out,
                         rk_mask_stats *stats);

int rk_sketches_mask(rk_ctx *ctx, const rk_sketches *queries, const rk_index *idx, const rk_mask_rule *rule, rk_sketches **out, rk_mask_stats *stats)
{
    return sketches_mask(ctx, queries, idx, rule, false, out, stats);
}

int rk_sketches_mask_counts(rk_ctx *ctx, const rk_sketches *queries, const rk_index *idx, const rk_mask_rule *rule, rk_sketches **out, rk_mask_stats *stats)
{
    return sketches_mask(ctx, queries, idx, rule, true, out, stats);
}

// rk_sketches_mask, and with_counts rk_sketches_mask_counts: every survivor keeps its count
static int sketches_mask(rk_ctx *ctx, const rk_sketches *queries, const rk_index *idx, const rk_mask_rule *rule, bool with_counts, rk_sketches **out,
                         rk_mask_stats *stats)
{
    if (!ctx || !queries || !idx || !rule || !out) return RK_ERR_ARG;
    const char *const who = with_counts ? "rk_sketches_mask_counts" : "rk_sketches_mask";
    if (with_counts && !queries->d_counts) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "%s: the query sketches carry no counts (rk_sketches_has_counts)", who);
    if (rule->min_refs > rule->max_refs) return rk_fail(ctx, RK_ERR_ARG, "%s: min_refs is above max_refs", who);
    if (queries->wide != idx->wide) return rk_fail(ctx, RK_ERR_ARG, "query sketches and index use different hash widths");
    if (!idx->d_postings || !idx->d_upos || idx->n_shards > 1)
        return rk_fail(ctx, RK_ERR_ARG, "%s: an index without all posting lists (rk_index_join_shard, one hash range of a sharded build)", who);
    rk_mask_stats st;
    memset(&st, 0, sizeof st);
    const TimedSpan span{ctx, RK_MS_MASK};
    span.clear();
    rk_sketches *s = nullptr;
    if (queries->n) {
        fill_geometry(&st, queries->total);
        if (rk_switched_off("RK_MASK_DEVICE")) {
            st.path = 2;
            RK_TRY(queries->wide ? mask_on_host<uint64_t>(ctx, queries, idx, rule, with_counts, &st, &s)
                                 : mask_on_host<uint32_t>(ctx, queries, idx, rule, with_counts, &st, &s));
        } else {
            st.path = 1;
            RK_TRY(mask_on_device(ctx, queries, idx, rule, with_counts, &st, &s));
        }
    }
    *out = s;
    if (stats) *stats = st;
    return RK_OK;
}

}  // extern "C"
