// rk_index_fast.inc -- the fast path of rk_index_build (included by rk_index.hip inside its anonymous namespace).
//
// Replaces the device-wide radix sort of (hash, source element) + 7 gather/scatter kernels of the general path by a
// two-level bucket sort whose second level runs entirely in LDS and emits everything the index needs while the
// bucket is on chip:
//
//   k_chunk_first   which genome every chunk of 64 K source elements starts in
//   k_range_filter  (range passes only: a shard of a multi-GPU build, a pass of a collection beyond 2^15 buckets) the pass's
//                   elements written dense -- the kernels below then partition those instead of walking the sketches
//   k_part_hist     per chunk of ~64 K source elements: how many fall into each of the 2^B buckets (top B hash bits)
//   k_part_colscan  per bucket: running sum over the chunks  -> where each chunk's run starts inside the bucket
//   k_part_starts   one workgroup: exclusive scan of the bucket sizes -> bucket starts (and the overflow check)
//   k_part_scatter  the chunks again: 8-byte keys (hash low bits | internal genome | position in its sketch) to their
//                   bucket; every (chunk, bucket) run has its own reserved stretch: no global atomics, deterministic
//   k_bucket_emit   one workgroup per bucket (<= 4,096 keys, in registers + one LDS array): counting sort by the next 10 hash bits, rank sort
//                   inside each of the 1,024 sub-buckets (a handful of keys), then -- the bucket sorted by (hash, genome) --
//                   postings, list heads, and for every element the slice record of its "later genomes" in final form
//                   (compact: first genome + bitmask; else the posting range), written to the element's place in its row
//   k_heads_scan / k_heads_place   distinct hashes and posting offsets compacted over the buckets
//   k_row_counts2 / k_row_scan / k_row_place2   empty slices dropped, covered ones last (as in the general path)
//
// Conditions: 32-bit hashes, set sketches (strictly ascending: no genome twice in a list), fewer than 2^31 postings,
// key fields that fit 64 bits, at most 2^15 buckets and no bucket beyond the LDS capacity (a hash space so skewed that
// one bucket holds more than ~2.7x its share).  Anything else -- decided on the host before the first launch or by a
// flag the kernels raise -- takes the general path.
// HBM-bound streaming + LDS work; integer/index arithmetic, no MFMA.

constexpr uint32_t kBucketCap = 4096;       // keys of one bucket in LDS (2 x 8 B x 4,096 = 64 KiB: two workgroups per CU)
constexpr uint32_t kBucketTarget = 1536;    // mean bucket size aimed for (the cap tolerates a 2.7x heavier bucket)
constexpr int kMaxBucketBits = 15;          // 2^15 x 4 B of LDS counters in the partition kernels
constexpr uint32_t kPartThreads = 1024;
constexpr uint32_t kPartChunk = 65536;      // source elements per partition workgroup (16 waves x 4,096)
constexpr int kSubBits = 10;                // sub-buckets of the LDS counting sort

enum : unsigned long long { kFastOverflow = 1, kFastBadHash = 2 };

// Workgroup b runs on XCD b % 8 (round-robin dispatch), and the XCDs' L2 caches do not see each other's dirty lines.
// The partition and the emission scatter 8-byte records whose NEIGHBOURS in memory are written by the neighbouring chunk
// (the next 64 bytes of a bucket) or by the next ~100 buckets (the next records of a genome's row): with neighbouring
// items on different XCDs every cache line leaves eight L2s as eight partial writes.  This maps the workgroups of one XCD
// onto a contiguous range of items, so that a line is completed inside one L2.  xcd_map == 0: identity (RK_INDEX_XCD=0).
__device__ inline uint32_t xcd_item(uint32_t b, uint32_t n, int xcd_map)
{
    if (!xcd_map) return b;
    const uint32_t x = b & 7u, i = b >> 3, q = n >> 3, r = n & 7u;   // XCD x runs q + (x < r) of the n workgroups
    return x * q + min(x, r) + i;
}

struct FastArgs {
    const void *hashes;         // the caller's CSR: u32 hashes, or u64 (64-bit hash layout: the kernels are templated on HT)
    const uint64_t *off;
    const uint32_t *orig;       // walking order -> caller's genome (null: the walk IS the caller's order)
    const uint64_t *off_new;    // CSR offsets in walking order (u64[N+1])
    uint32_t n_genomes;
    uint64_t H;
    int hash_bits, low_bits, gb, rb;   // key = hash_low << (gb + rb) | genome << rb | position
    int xcd_map;                // xcd_item()
    uint32_t nb;                // buckets
    uint32_t n_chunks;
    // (round 5) one RANGE of the hash space per build pass: range_bits > 0 keeps only the hashes whose top range_bits bits (of
    // hash_bits) equal range_id -- a shard of a multi-GPU build, or one pass of a collection too big for 2^15 buckets; buckets
    // and low bits then apply to the remaining hash_bits - range_bits bits
    int range_bits;
    uint32_t range_id;
    uint64_t keys_cap;          // what the key buffers of a pass hold (== H without ranges)
    // (round 5) a range pass over a FILTERED source: k_range_filter has written the pass's elements -- (hash inside the range) << gb |
    // genome, dense, in any order -- and the partition kernels read those instead of walking the sketches (range_bits is then 0 and
    // hash_bits the bits inside the range: nothing is left to test); *n_filtered of them, known on the device only
    const unsigned long long *filtered;
    const unsigned long long *n_filtered;
    __device__ uint64_t source_elements() const { return filtered ? min((uint64_t)*n_filtered, keys_cap) : H; }
    __device__ bool in_range(unsigned long long h) const { return range_bits == 0 || (uint32_t)(h >> (hash_bits - range_bits)) == range_id; }
    __device__ uint32_t bucket_of(unsigned long long h) const
    {
        return (uint32_t)((range_bits ? (h & ((1ULL << (hash_bits - range_bits)) - 1ULL)) : h) >> low_bits);
    }
};

// chunk c of the internal-order element space starts inside genome first[c] (largest i with off_new[i] <= c * kPartChunk);
// first[n_chunks] = the last genome
// (round 4: the same launch zeroes `zero_words` 8-byte words at `zero` -- the result record and the partition's cursors --:
// a hipMemsetAsync of that size is two dispatches of ~4 us each in front of this one)
__global__ void k_chunk_first(const uint64_t *off_new, uint32_t n_genomes, uint32_t n_chunks, uint32_t *first, unsigned long long *zero,
                              uint32_t zero_words)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t w = c; w < zero_words; w += gridDim.x * blockDim.x) zero[w] = 0;
    if (c > n_chunks) return;
    if (c == n_chunks) { first[c] = n_genomes - 1; return; }
    const uint64_t e = (uint64_t)c * kPartChunk;
    uint32_t lo = 0, hi = n_genomes;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off_new[mid] <= e) lo = mid; else hi = mid;
    }
    first[c] = lo;
}

// Where the genomes of a chunk end (in the internal-order element space) and where their hashes lie in the caller's
// array (delta: source element = internal element + delta).  A lane steps to its next genome once per ~sketch/64
// steps, but in almost EVERY step some lane of the wave does: those look-ups must not be chains of global loads
// (measured: 48 us for a pass that only reads 49 MB), so a workgroup stages the bounds of its chunk's genomes in LDS.
constexpr uint32_t kStageGenomes = 1024;
struct StagedGenomes {   // LDS, genomes ga .. ga + n - 1
    const uint64_t *end, *delta;
    uint32_t ga;
    __device__ uint64_t end_of(uint32_t i) const { return end[i - ga]; }
    __device__ uint64_t delta_of(uint32_t i) const { return delta[i - ga]; }
};
struct GlobalGenomes {
    const FastArgs *a;
    __device__ uint64_t end_of(uint32_t i) const { return a->off_new[i + 1]; }
    __device__ uint64_t delta_of(uint32_t i) const { return a->off[a->orig ? a->orig[i] : i] - a->off_new[i]; }
};

// Every wave of the workgroup walks a contiguous stretch of the chunk [c0, c1) of the internal-order element space,
// 64 elements per step; f(hash, internal genome, position inside its sketch).  ga / gb: first and last genome of the chunk.
template <class HT, class V, class F>
__device__ inline void walk_chunk(const FastArgs &a, const V &view, uint32_t ga, uint32_t gb, uint64_t c0, uint64_t c1, F f)
{
    const HT *hashes = static_cast<const HT *>(a.hashes);
    constexpr int D = 4;  // steps in flight: the hash loads of D steps are issued before the first is used
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint64_t cw = (((c1 - c0) + nw - 1) / nw + 63) & ~63ULL;
    const uint64_t w0 = c0 + (uint64_t)wave * cw, w1 = min(c1, w0 + cw);
    if (w0 >= w1) return;
    uint32_t lo = ga, hi = gb;  // first genome whose end lies beyond w0 (wave-uniform)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (view.end_of(mid) <= w0) lo = mid + 1; else hi = mid;
    }
    uint32_t i = lo;
    uint64_t i_end = view.end_of(i), delta = view.delta_of(i);
    uint64_t i_beg = a.off_new[i];
    for (uint64_t base = w0; base < w1; base += 64 * D) {
        uint32_t gi[D], ri[D];
        HT hv[D];
        bool ok[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint64_t e = base + 64 * d + lane;
            ok[d] = e < w1;
            gi[d] = ri[d] = hv[d] = 0;
            if (ok[d]) {
                while (e >= i_end) {  // next genome (empty sketches are stepped over)
                    i++;
                    i_beg = i_end;
                    i_end = view.end_of(i);
                    delta = view.delta_of(i);
                }
                gi[d] = i;
                ri[d] = (uint32_t)(e - i_beg);
                hv[d] = hashes[e + delta];
            }
        }
#pragma unroll
        for (int d = 0; d < D; d++)
            if (ok[d]) f(hv[d], gi[d], ri[d]);
    }
}

// stages the chunk's genome bounds (when they fit) and walks it
template <class HT, class F>
__device__ inline void walk_chunk_staged(const FastArgs &a, uint32_t chunk, const uint32_t *chunk_first, uint64_t *stage /* LDS, 2 * kStageGenomes */, F f)
{
    const uint64_t c0 = (uint64_t)chunk * kPartChunk, c1 = min(a.H, c0 + kPartChunk);
    const uint32_t ga = chunk_first[chunk], gb = chunk_first[chunk + 1];
    const uint32_t ng = gb - ga + 1;
    if (ng <= kStageGenomes) {
        for (uint32_t k = threadIdx.x; k < ng; k += blockDim.x) {
            const uint32_t i = ga + k;
            stage[k] = a.off_new[i + 1];
            stage[kStageGenomes + k] = a.off[a.orig ? a.orig[i] : i] - a.off_new[i];
        }
        __syncthreads();
        StagedGenomes v{stage, stage + kStageGenomes, ga};
        walk_chunk<HT>(a, v, ga, gb, c0, c1, f);
    } else {
        GlobalGenomes v{&a};
        walk_chunk<HT>(a, v, ga, gb, c0, c1, f);
    }
}

// (round 5) One range of the hash space out of a collection that has several (a shard of a multi-GPU build, a pass of a collection
// beyond 2^15 buckets): until now every partition kernel of the pass walked ALL hashes and dropped 7 in 8 -- the count matrix had a
// row per 64 K source elements whatever the range kept (1 GB written and read twice at 500,000 genomes), and the coarse pass sorted
// tiles that were one-eighth full (runs of 2 keys).  This kernel reads the hashes once and writes the range's elements DENSE; the
// partition then runs over those as over a collection of that size.  A workgroup counts its chunk's elements inside the range
// (wave by wave, flat), reserves their place with ONE atomic, and walks the chunk again (from the cache) with the genome bounds:
// every wave writes its stretch's elements in order, a step of 64 lanes as one contiguous run.
// (workgroups of 256 threads, four per chunk: the renumbering's kernels run beside this one, and a workgroup that needs a whole CU to
// itself waits until they have drained -- measured: 1.7 ms beside k_minhash_insert, 0.64 ms alone)
constexpr uint32_t kFilterSplit = 4, kFilterThreads = 256;
template <class HT>
__global__ __launch_bounds__(kFilterThreads) void k_range_filter(FastArgs a, const uint32_t *chunk_first, unsigned long long *out, unsigned long long *cursor,
                                                               BuildResult *res)
{
    __shared__ uint64_t stage[kStageGenomes];
    __shared__ uint32_t wave_cnt[kFilterThreads / 64];
    __shared__ unsigned long long s_base;
    const HT *hashes = static_cast<const HT *>(a.hashes);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr uint32_t nw = kFilterThreads / 64;
    constexpr uint32_t kSteps = kPartChunk / (64 * nw * kFilterSplit);   // a wave's stretch: 64 steps of 64 lanes
    // (32-bit hashes: a lane keeps its 64 hashes in registers between the count and the walk -- all 64 loads are in flight at once and
    // nothing is read twice; 64-bit hashes are read again, from the cache)
    constexpr bool kInRegs = sizeof(HT) == 4;
    const uint32_t item = xcd_item(blockIdx.x, gridDim.x, a.xcd_map);   // kFilterSplit workgroups per chunk (they share its genome bounds)
    const uint32_t chunk = item / kFilterSplit, part = item % kFilterSplit;
    const uint64_t c0 = (uint64_t)chunk * kPartChunk, c1 = min(a.H, c0 + kPartChunk);
    const uint64_t w0 = min(c1, c0 + (uint64_t)(part * nw + wave) * (64 * kSteps)), w1 = min(c1, w0 + 64 * kSteps);
    const uint32_t ga = chunk_first[chunk], gb = chunk_first[chunk + 1];
    const uint32_t ng = gb - ga + 1;
    const bool staged = ng <= kStageGenomes;
    if (staged)
        for (uint32_t k = tid; k < ng; k += kFilterThreads) stage[k] = a.off_new[ga + k + 1];
    HT hv[kInRegs ? kSteps : 1];
    uint32_t cnt = 0;
    bool bad = false;
    auto outside = [&](HT h) { return a.hash_bits < (int)(8 * sizeof(HT)) && (h >> a.hash_bits) != 0; };
    // (an element beyond the stretch's end is given a hash of the neighbouring range: nothing below asks where the stretch ends)
    const HT skip = (HT)((unsigned long long)(a.range_id ^ 1u) << (a.hash_bits - a.range_bits));
    if (kInRegs) {
        const HT *src = hashes + w0 + lane;
        if (w1 - w0 == 64 * kSteps) {
#pragma unroll
            for (uint32_t j = 0; j < kSteps; j++) hv[kInRegs ? j : 0] = src[64 * j];
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kSteps; j++) hv[kInRegs ? j : 0] = w0 + 64 * j + lane < w1 ? src[64 * j] : skip;
        }
#pragma unroll
        for (uint32_t j = 0; j < kSteps; j++) {
            const HT h = hv[kInRegs ? j : 0];
            if (outside(h)) bad = true;   // outside the hash space: general path
            else if (a.in_range(h)) cnt++;
        }
    } else {
        constexpr int D = 8;
        for (uint64_t base = w0 + lane; base < w1; base += 64 * D) {
            HT t[D];
#pragma unroll
            for (int d = 0; d < D; d++) t[d] = base + 64 * d < w1 ? hashes[base + 64 * d] : (HT)0;
#pragma unroll
            for (int d = 0; d < D; d++)
                if (base + 64 * d < w1) {
                    if (outside(t[d])) bad = true;
                    else if (a.in_range(t[d])) cnt++;
                }
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
    if (lane == 0) wave_cnt[wave] = cnt;
    if (bad) atomicOr(&res->flags, kFastBadHash);
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < nw; w++) all += wave_cnt[w];
        unsigned long long at = all ? atomicAdd(cursor, (unsigned long long)all) : 0ULL;
        if (at + all > a.keys_cap) {   // (the range holds more than estimated: the pass stands still, the host decides)
            atomicOr(&res->flags, kFastOverflow);
            at = ~0ULL;
        }
        s_base = at;
    }
    __syncthreads();
    if (s_base == ~0ULL || w0 >= w1 || cnt == 0) return;   // (cnt: the wave's sum, uniform)
    unsigned long long at = s_base;
    for (uint32_t w = 0; w < wave; w++) at += wave_cnt[w];
    auto end_of = [&](uint32_t i) -> uint64_t { return staged ? stage[i - ga] : a.off_new[i + 1]; };
    uint32_t i;
    {
        uint32_t lo = ga, hi = gb;   // first genome whose end lies beyond w0 (wave-uniform)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (end_of(mid) <= w0) lo = mid + 1; else hi = mid;
        }
        i = lo;
    }
    uint64_t i_end = end_of(i);
    const unsigned long long eff_mask = (1ULL << (a.hash_bits - a.range_bits)) - 1ULL;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    // one step: 64 consecutive elements, the kept ones leave as one contiguous run (all lanes arrive: the ballot sees the wave)
    auto step = [&](uint64_t e, HT h) {
        const bool keep = !outside(h) && a.in_range(h);
        const unsigned long long m = __ballot(keep);
        if (!m) return;
        if (keep) {
            while (e >= i_end) {   // next genome (empty sketches are stepped over)
                i++;
                i_end = end_of(i);
            }
            out[at + (uint32_t)__popcll(m & lt)] = (((unsigned long long)h & eff_mask) << a.gb) | i;
        }
        at += (uint32_t)__popcll(m);
    };
    if (kInRegs) {
#pragma unroll
        for (uint32_t j = 0; j < kSteps; j++) {
            step(w0 + 64 * j + lane, hv[kInRegs ? j : 0]);
            __builtin_amdgcn_sched_barrier(0);   // (step by step: scheduled across steps the ballots and their masks spill)
        }
    } else {
        constexpr int D = 8;
        for (uint64_t base = w0; base < w1; base += 64 * D) {   // (wave-uniform trips)
            HT t[D];
#pragma unroll
            for (int d = 0; d < D; d++) t[d] = base + 64 * d + lane < w1 ? hashes[base + 64 * d + lane] : skip;
#pragma unroll
            for (int d = 0; d < D; d++) step(base + 64 * d + lane, t[d]);
        }
    }
}

template <class HT>
__global__ __launch_bounds__(kPartThreads) void k_part_hist(FastArgs a, const uint32_t *chunk_first, uint32_t *matrix, BuildResult *res)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t part_lds[];
    uint64_t *stage = reinterpret_cast<uint64_t *>(part_lds + a.nb);
    for (uint32_t b = threadIdx.x; b < a.nb; b += kPartThreads) part_lds[b] = 0;
    __syncthreads();
    bool bad = false;
    const uint32_t chunk = xcd_item(blockIdx.x, gridDim.x, a.xcd_map);
    auto count = [&](HT h, uint32_t, uint32_t) {
        if (a.hash_bits < (int)(8 * sizeof(HT)) && (h >> a.hash_bits)) { bad = true; return; }  // outside the hash space: general path
        if (!a.in_range(h)) return;
        atomicAdd(&part_lds[a.bucket_of(h)], 1u);
    };
    if (a.filtered) {
        if (!res->flags) {   // (a filter that ran out of space left holes: nothing may be read as a key)
            const uint64_t nf = a.source_elements();
            const uint64_t c0 = min(nf, (uint64_t)chunk * kPartChunk), c1 = min(nf, c0 + kPartChunk);
            constexpr int D = 8;
            for (uint64_t base = c0 + threadIdx.x; base < c1; base += (uint64_t)kPartThreads * D) {
                unsigned long long kv[D];
#pragma unroll
                for (int d = 0; d < D; d++) kv[d] = base + (uint64_t)d * kPartThreads < c1 ? a.filtered[base + (uint64_t)d * kPartThreads] : 0ULL;
#pragma unroll
                for (int d = 0; d < D; d++)
                    if (base + (uint64_t)d * kPartThreads < c1) {
                        // (keys that came from another rank, rk_index_build_shard_keys: one outside the wire format -- a hash beyond the
                        // range's bits, a genome beyond the collection -- refuses the build instead of reaching past the counters)
                        const unsigned long long hb = kv[d] >> a.gb;
                        const uint32_t g = (uint32_t)(kv[d] & ((1ULL << a.gb) - 1ULL));
                        if ((a.hash_bits < 64 && (hb >> a.hash_bits)) || g >= a.n_genomes) bad = true;
                        else atomicAdd(&part_lds[(uint32_t)(hb >> a.low_bits)], 1u);
                    }
            }
        }
    } else if (!a.orig) {
        // the walk is the caller's CSR itself and a histogram does not ask whose hash it counts: a flat pass over the chunk's
        // elements, no genome bounds (round 4)
        const HT *hashes = static_cast<const HT *>(a.hashes);
        const uint64_t c0 = (uint64_t)chunk * kPartChunk, c1 = min(a.H, c0 + kPartChunk);
        constexpr int D = 8;
        for (uint64_t base = c0 + threadIdx.x; base < c1; base += (uint64_t)kPartThreads * D) {
            HT hv[D];
#pragma unroll
            for (int d = 0; d < D; d++) hv[d] = base + (uint64_t)d * kPartThreads < c1 ? hashes[base + (uint64_t)d * kPartThreads] : (HT)0;
#pragma unroll
            for (int d = 0; d < D; d++)
                if (base + (uint64_t)d * kPartThreads < c1) count(hv[d], 0, 0);
        }
    } else {
        walk_chunk_staged<HT>(a, chunk, chunk_first, stage, count);
    }
    if (bad) atomicOr(&res->flags, kFastBadHash);
    __syncthreads();
    uint32_t *row = matrix + (size_t)chunk * a.nb;
    for (uint32_t b = threadIdx.x; b < a.nb; b += kPartThreads) row[b] = part_lds[b];
}

// matrix[c][b] becomes the number of the bucket's keys that come from chunks before c; total[b] = the bucket's size.
// A workgroup of 1,024 threads owns 64 neighbouring buckets (coalesced rows) x 16 stretches of chunks
__global__ __launch_bounds__(1024) void k_part_colscan(uint32_t *matrix, uint32_t n_chunks, uint32_t nb, uint32_t *total)
{
    __shared__ uint32_t part[16][64];
    const uint32_t col = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * 64 + col;
    const uint32_t per = (n_chunks + 15) / 16;
    const uint32_t c0 = min(n_chunks, rg * per), c1 = min(n_chunks, c0 + per);
    uint32_t sum = 0;
    if (b < nb)
        for (uint32_t c = c0; c < c1; c++) sum += matrix[(size_t)c * nb + b];
    part[rg][col] = sum;
    __syncthreads();
    uint32_t run = 0, all = 0;
    for (uint32_t r = 0; r < 16; r++) {
        if (r < rg) run += part[r][col];
        all += part[r][col];
    }
    if (b < nb) {
        for (uint32_t c = c0; c < c1; c++) {
            const size_t at = (size_t)c * nb + b;
            const uint32_t v = matrix[at];
            matrix[at] = run;
            run += v;
        }
        if (rg == 0) total[b] = all;
    }
}

// single workgroup: bucket starts; raises the overflow flag when a bucket does not fit the LDS sort
// (big_list / n_big: buckets beyond the LDS sort are listed for k_bucket_heavy instead of refusing the whole build)
__global__ void k_part_starts(const uint32_t *total, uint32_t nb, uint32_t *bstart, BuildResult *res, unsigned long long *pass_base, unsigned long long keys_cap,
                              uint32_t *big_list, uint32_t *n_big)
{
    bool over = false;
    const uint32_t all = block_scan_sweeps<uint32_t>(
        nb, [&](uint32_t b) {
            const uint32_t v = total[b];
            if (v > kBucketCap) {
                if (big_list) big_list[atomicAdd(n_big, 1u)] = b;
                else over = true;
            }
            return v;
        },
        [&](uint32_t b, uint32_t before) { bstart[b] = before; });
    if (threadIdx.x == 0) {
        bstart[nb] = all;
        pass_base[1] = pass_base[0] + all;   // (where the next pass's postings start)
        if (all > keys_cap) over = true;     // (a range holds more keys than estimated: the passes behind stand still, the general path decides)
    }
    if (over) atomicOr(&res->flags, kFastOverflow);
}

template <class HT>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter(FastArgs a, const uint32_t *chunk_first, const uint32_t *matrix,
                                                               const uint32_t *bstart, unsigned long long *keys, const BuildResult *stop)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t part_lds[];
    if (a.range_bits && stop->flags) return;   // (a pass beyond its key buffer: k_part_starts)
    uint64_t *stage = reinterpret_cast<uint64_t *>(part_lds + a.nb);
    const uint32_t chunk = xcd_item(blockIdx.x, gridDim.x, a.xcd_map);
    const uint32_t *row = matrix + (size_t)chunk * a.nb;
    for (uint32_t b = threadIdx.x; b < a.nb; b += kPartThreads) part_lds[b] = bstart[b] + row[b];
    __syncthreads();
    const uint32_t low_mask = (1u << a.low_bits) - 1u;  // low_bits <= 31
    walk_chunk_staged<HT>(a, chunk, chunk_first, stage, [&](HT h, uint32_t g, uint32_t r) {
        if ((a.hash_bits < (int)(8 * sizeof(HT)) && (h >> a.hash_bits)) || !a.in_range(h)) return;  // (outside the hash space: flagged by k_part_hist, the result is discarded)
        const uint32_t pos = atomicAdd(&part_lds[a.bucket_of(h)], 1u);
        keys[pos] = ((unsigned long long)((uint32_t)h & low_mask) << (a.gb + a.rb)) | ((unsigned long long)g << a.rb) | (a.rb ? r : 0u);   // (rb == 0: tile records as the product, nobody needs the position)
    });
}

// ---- the partition in two passes (RK_INDEX_PART2, default on when the key has six spare bits and there are >= 128 buckets) ----
// k_part_scatter writes every key with a request of its own (64 lanes, 64 buckets): 12.2 M write requests at 10,000
// genomes, 160 us whatever the chunk size, and skipping the L2's write combining makes it three times worse -- it is the
// NUMBER of requests.  Here a workgroup collects 8,192 keys, sorts them in LDS by COARSE bucket (bucket >> 6: runs of
// 64 keys and more) and writes the runs coalesced into the chunk's own stretch of every coarse bucket (offsets from the
// same count matrix: no atomics, no new scan); a second pass sorts 8,192 keys of ONE coarse bucket by their fine bucket
// (runs of 128) and writes them to their final bucket, reserving the space of a run with one atomic on the bucket's
// cursor.  The order of the keys inside a bucket is whatever comes: k_bucket_emit sorts them.
constexpr uint32_t kTileKeys = 8192;   // keys a workgroup sorts at a time (8 per thread)
constexpr uint32_t kFineBits = 6;      // fine buckets per coarse bucket: 64
constexpr uint32_t kMaxCoarse = (1u << kMaxBucketBits) >> kFineBits;

// one tile in LDS: keys -> sorted by bin -> runs written to out[gbase[bin] + ...].  Called by all threads; bins < n_bins.
// key[i] / bin[i] / ok[i]: the thread's eight keys.  hist, lstart, gbase, cursor: n_bins words each; reserve(bin, count)
// returns where the tile's run of that bin goes (called by the lanes of wave 0, bins in order).
template <uint32_t T, class BinT, class Reserve>
__device__ inline void sort_tile_and_write(const unsigned long long (&key)[8], const uint32_t (&bin)[8], const bool (&ok)[8], uint32_t n_bins,
                                           unsigned long long *sorted, BinT *sorted_bin, uint32_t *hist, uint32_t *lstart,
                                           uint32_t *gbase, uint32_t *cursor, unsigned long long *out, Reserve reserve)
{
    // (hist[0 .. n_bins) is zero on entry: the caller clears it once, wave 0 clears it again below.  Three barriers per
    // tile: the write-out of one tile runs into the histogram of the next -- they share nothing)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (ok[i]) atomicAdd(&hist[bin[i]], 1u);
    __syncthreads();
    if (tid < 64) {   // wave 0: exclusive scan over the bins, eight stretches of 64
        uint32_t running = 0;
        for (uint32_t b0 = 0; b0 < n_bins; b0 += 64) {
            const uint32_t b = b0 + lane;
            const uint32_t cnt = b < n_bins ? hist[b] : 0u;
            uint32_t incl = cnt;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if ((int)lane >= o) incl += up;
            }
            if (b < n_bins) {
                lstart[b] = running + incl - cnt;
                cursor[b] = running + incl - cnt;
                gbase[b] = cnt ? reserve(b, cnt) : 0u;
                hist[b] = 0;
            }
            running += (uint32_t)__shfl((int)incl, 63);
        }
        if (lane == 0) hist[n_bins] = running;   // keys in the tile
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (ok[i]) {
            const uint32_t pos = atomicAdd(&cursor[bin[i]], 1u);
            sorted[pos] = key[i];
            sorted_bin[pos] = (BinT)bin[i];
        }
    __syncthreads();
    const uint32_t n_tile = hist[n_bins];
    for (uint32_t q = tid; q < n_tile; q += T) {
        const uint32_t b = sorted_bin[q];
        out[(size_t)gbase[b] + (q - lstart[b])] = sorted[q];
    }
}

// kCoarseThreads threads per workgroup, 1,024 / kCoarseThreads workgroups share a chunk (its 16 wave stretches dealt among
// them) and sort 8 x kCoarseThreads keys at a time: 256 threads when there are at most 128 coarse buckets (runs of 16 keys and
// more; three workgroups fit a CU and all CUs have work), 1,024 beyond (512 coarse buckets at 50,000 genomes: a tile of
// 2,048 keys would cut the runs to 4 keys)
constexpr size_t part2_lds(uint32_t threads) { return (size_t)threads * 8 * 8 + (size_t)threads * 8 * 2 + 2 * kStageGenomes * 8 + (5 * kMaxCoarse + 16) * 4; }

template <uint32_t kCoarseThreads, class HT>
__global__ __launch_bounds__(kCoarseThreads) void k_part_coarse(FastArgs a, const uint32_t *chunk_first, const uint32_t *matrix,
                                                                const uint32_t *bstart, uint32_t *seg_taken, unsigned long long *mid, const BuildResult *stop)
{
    constexpr uint32_t kCoarseSubs = kPartThreads / kCoarseThreads, kCoarseTile = 8 * kCoarseThreads;
    extern __shared__ __attribute__((aligned(16))) unsigned char p2_lds[];
    if ((a.range_bits || a.filtered) && stop->flags) return;   // (a pass beyond its key buffer: k_part_starts / k_range_filter)
    unsigned long long *sorted = reinterpret_cast<unsigned long long *>(p2_lds);
    uint16_t *sorted_bin = reinterpret_cast<uint16_t *>(sorted + kCoarseTile);
    uint64_t *stage = reinterpret_cast<uint64_t *>(sorted_bin + kCoarseTile);
    uint32_t *hist = reinterpret_cast<uint32_t *>(stage + 2 * kStageGenomes);   // n_coarse + 1 words
    uint32_t *lstart = hist + kMaxCoarse + 16, *gbase = lstart + kMaxCoarse, *cursor = gbase + kMaxCoarse, *seg = cursor + kMaxCoarse;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    // (several small workgroups per chunk instead of one of 1,024 threads: three of them fit a CU and their phases --
    // histogram, scan, ranks, write-out, each behind a barrier -- overlap; all CUs have work, not 187 of 256)
    const uint32_t item = xcd_item(blockIdx.x, gridDim.x, a.xcd_map);
    const uint32_t chunk = item / kCoarseSubs, sub = item % kCoarseSubs;
    const uint32_t wave = sub * (kCoarseThreads / 64) + (tid >> 6), nw = kPartThreads / 64;   // this wave's stretch among the chunk's 16
    const uint32_t n_coarse = a.nb >> kFineBits;
    // where this chunk's keys of every coarse bucket go: behind those of the chunks before it (the sub-workgroups of a
    // chunk share the stretch: a run's place in it comes from an atomic on the chunk's counter of that bucket)
    for (uint32_t cb = tid; cb < n_coarse; cb += kCoarseThreads) {
        hist[cb] = 0;
        const uint32_t *row = matrix + (size_t)chunk * a.nb + ((size_t)cb << kFineBits);
        uint32_t before = 0;
        for (uint32_t f = 0; f < (1u << kFineBits); f++) before += row[f];
        seg[cb] = bstart[cb << kFineBits] + before;
    }
    uint32_t *taken = seg_taken + (size_t)chunk * n_coarse;
    // the chunk's genome bounds (as walk_chunk_staged)
    const uint64_t n_src = a.source_elements();
    const uint64_t c0 = min(n_src, (uint64_t)chunk * kPartChunk), c1 = min(n_src, c0 + kPartChunk);
    const uint32_t ga = a.filtered ? 0u : chunk_first[chunk], gb = a.filtered ? 0u : chunk_first[chunk + 1];
    const uint32_t ng = gb - ga + 1;
    const bool staged = ng <= kStageGenomes;
    if (staged && !a.filtered)
        for (uint32_t k = tid; k < ng; k += kCoarseThreads) {
            const uint32_t i = ga + k;
            stage[k] = a.off_new[i + 1];
            stage[kStageGenomes + k] = a.off[a.orig ? a.orig[i] : i] - a.off_new[i];
        }
    __syncthreads();
    auto end_of = [&](uint32_t i) -> uint64_t { return staged ? stage[i - ga] : a.off_new[i + 1]; };
    auto delta_of = [&](uint32_t i) -> uint64_t { return staged ? stage[kStageGenomes + (i - ga)] : a.off[a.orig ? a.orig[i] : i] - a.off_new[i]; };
    // every wave walks its own stretch of the chunk, 512 elements per tile (as walk_chunk)
    const uint64_t cw = (((c1 - c0) + nw - 1) / nw + 63) & ~63ULL;
    const uint64_t w0 = c0 + (uint64_t)wave * cw, w1 = min(c1, w0 + cw);
    uint32_t i = ga;
    uint64_t i_end = 0, i_beg = 0, delta = 0;
    if (w0 < w1 && !a.filtered) {
        uint32_t lo = ga, hi = gb;
        while (lo < hi) {
            const uint32_t midg = (lo + hi) >> 1;
            if (end_of(midg) <= w0) lo = midg + 1; else hi = midg;
        }
        i = lo;
        i_end = end_of(i);
        delta = delta_of(i);
        i_beg = a.off_new[i];
    }
    const uint32_t low_mask = (1u << a.low_bits) - 1u;
    // the hashes of the NEXT tile are on their way while this one is sorted and written
    const HT *hashes = static_cast<const HT *>(a.hashes);
    HT hN[8];
    uint32_t gN[8], rN[8];
    bool okN[8];
    auto request = [&](uint64_t tb) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t e = w0 + tb + 64 * (uint64_t)j + lane;
            okN[j] = tb < cw && e < w1;
            hN[j] = 0;
            gN[j] = rN[j] = 0;
            if (a.filtered) {   // (uniform) the element IS (hash inside the range, genome)
                if (okN[j]) {
                    const unsigned long long k = a.filtered[e];
                    hN[j] = (HT)(k >> a.gb);
                    gN[j] = (uint32_t)k & ((1u << a.gb) - 1u);
                }
            } else if (okN[j]) {
                while (e >= i_end) {   // next genome (empty sketches are stepped over)
                    i++;
                    i_beg = i_end;
                    i_end = end_of(i);
                    delta = delta_of(i);
                }
                gN[j] = i;
                rN[j] = (uint32_t)(e - i_beg);
                hN[j] = hashes[e + delta];
            }
        }
    };
    request(0);
    for (uint64_t tb = 0; tb < cw; tb += 512) {   // (the same trips for every wave: the tile is the workgroup's)
        unsigned long long key[8];
        uint32_t bin[8];
        bool ok[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const HT h = hN[j];
            ok[j] = okN[j] && !(a.hash_bits < (int)(8 * sizeof(HT)) && (h >> a.hash_bits)) && a.in_range(h);   // (outside the hash space: flagged by k_part_hist, the result is discarded)
            const uint32_t b = ok[j] ? a.bucket_of(h) : 0u;
            bin[j] = b >> kFineBits;
            key[j] = ((unsigned long long)(b & ((1u << kFineBits) - 1u)) << (64 - kFineBits)) |
                     ((unsigned long long)((uint32_t)h & low_mask) << (a.gb + a.rb)) | ((unsigned long long)gN[j] << a.rb) | (a.rb ? rN[j] : 0u);
        }
        request(tb + 512);
        sort_tile_and_write<kCoarseThreads>(key, bin, ok, n_coarse, sorted, sorted_bin, hist, lstart, gbase, cursor, mid, [&](uint32_t b, uint32_t cnt) {
            if (kCoarseSubs == 1) {   // the chunk is this workgroup's alone (and only this lane of wave 0 touches seg[b])
                const uint32_t at = seg[b];
                seg[b] = at + cnt;
                return at;
            }
            return seg[b] + atomicAdd(&taken[b], cnt);
        });
    }
}

// pass two: the keys of coarse bucket blockIdx.x, tiles blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(kPartThreads) void k_part_fine(FastArgs a, const uint32_t *bstart, const unsigned long long *mid,
                                                            unsigned long long *keys, uint32_t *fine_cursor, const BuildResult *stop)
{
    if ((a.range_bits || a.filtered) && stop->flags) return;   // (a pass beyond its key buffer: k_part_starts / k_range_filter)
    __shared__ __attribute__((aligned(16))) unsigned long long sorted[kTileKeys];
    __shared__ uint8_t sorted_bin[kTileKeys];   // (64 bins: a byte each, and two workgroups fit a CU)
    __shared__ uint32_t hist[(1u << kFineBits) + 1], lstart[1u << kFineBits], gbase[1u << kFineBits], cursor[1u << kFineBits];
    const uint32_t tid = threadIdx.x;
    const uint32_t cb = blockIdx.x;
    const uint32_t r0 = bstart[cb << kFineBits], r1 = bstart[(cb + 1) << kFineBits];
    const unsigned long long strip = ~0ULL >> kFineBits;
    if (tid < (1u << kFineBits)) hist[tid] = 0;
    __syncthreads();
    for (uint32_t t0 = r0 + blockIdx.y * kTileKeys; t0 < r1; t0 += gridDim.y * kTileKeys) {
        unsigned long long key[8];
        uint32_t bin[8];
        bool ok[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t q = t0 + (uint32_t)j * kPartThreads + tid;
            ok[j] = q < r1 && q - t0 < kTileKeys;
            const unsigned long long k = ok[j] ? mid[q] : 0ULL;
            bin[j] = (uint32_t)(k >> (64 - kFineBits));
            key[j] = k & strip;
        }
        sort_tile_and_write<kPartThreads>(key, bin, ok, 1u << kFineBits, sorted, sorted_bin, hist, lstart, gbase, cursor, keys, [&](uint32_t b, uint32_t cnt) {
            const uint32_t fine = (cb << kFineBits) + b;
            return bstart[fine] + atomicAdd(&fine_cursor[fine], cnt);
        });
    }
}

// Slice records in the raw (one per source element) array carry their class: empty (0, 0); compact (bit 31 | first genome,
// bitmask with bit 0 set) -- covered: bit 0 cleared; posting range (x, y | near flag), x < y < 2^30 -- covered: bit 30 of x set.
// (near flag, bit 31 of y, also in the final record: the range's first genome lies within 32 ids of the element's own --
// only then can the range have members inside the window of rk_near_kernel, which otherwise never loads a posting for it)
__device__ inline uint8_t slice_class2(uint2 r)
{
    if ((r.x | r.y) == 0) return kEmpty;
    if (r.x >> 31) return (r.y & 1u) ? kOpen : kCovered;
    return (r.x >> 30) ? kCovered : kOpen;
}
__device__ inline uint2 slice_final2(uint2 r)
{
    if (r.x >> 31) return make_uint2(r.x, r.y | 1u);
    return make_uint2(r.x & 0x3FFFFFFFu, r.y);
}

struct EmitArgs {
    const unsigned long long *keys;
    const uint32_t *bstart;
    const uint64_t *off_new;          // CSR offsets in INTERNAL genome order (where an element's slice record goes)
    const uint32_t *inv;              // the keys carry the caller's genome index: inv[caller] = internal id (null: identity)
    const uint2 *tab;                 // with inv: tab[caller] = (internal id, its CSR offset in internal order) -- one gather instead of two dependent ones
    int low_bits, gb, rb;
    uint32_t nb;
    uint32_t *postings;
    uint32_t *tmp_uhash, *tmp_upos;   // list heads of bucket b at [bstart[b], bstart[b] + ucount[b])
    unsigned long long *tmp_uhash64;  // 64-bit hash layout: the list heads' hashes go here instead of tmp_uhash
    uint32_t *ucount;
    uint2 *self_raw;
    BuildResult *res;
    int xcd_map;  // xcd_item()
    int debug;   // developer ablations (RK_INDEX_DEBUG): 1 no slice scatter, 2 no posting / head stores, 4 no emission at all
};

// One workgroup of T threads per bucket.  Every thread keeps its (up to kBucketCap / T) keys in registers: ONE LDS
// array is enough -- sub-bucketed, then ranked in place (all ranks are known before the first key moves).  What is sorted
// is (hash_low, genome) only -- K = u32 when those fit 32 bits, the usual case --: the position of an element inside its
// sketch is needed by nobody but the thread that loaded it, which also requested the element's row offset as soon as
// the key arrived and writes the element's slice record.  Postings and list heads leave in sorted order, coalesced.
template <int T, class K>
__global__ __launch_bounds__(T, 8) void k_bucket_emit(EmitArgs a)
{
    constexpr uint32_t NW = T / 64, EPT = kBucketCap / T;
    constexpr uint32_t kSub = 1u << kSubBits;
    static_assert(kSub <= 4 * T, "the sub-bucket scan takes at most four entries per thread");
    __shared__ __attribute__((aligned(16))) K S[kBucketCap];
    __shared__ uint16_t hd[kBucketCap + 2];   // hd[i] = position of the i-th list head, hd[U] = n
    // sub-bucket starts + cursors while sorting; afterwards the list number of every sorted position
    __shared__ __attribute__((aligned(16))) uint32_t sb[2 * kSub + 2];
    __shared__ uint32_t wave_part[NW];
    uint32_t *sb_start = sb, *sb_cur = sb + kSub + 1;
    uint16_t *gidx = reinterpret_cast<uint16_t *>(sb);
    static_assert(sizeof(sb) >= kBucketCap * sizeof(uint16_t), "gidx overlays the sub-bucket arrays");
    const uint32_t b = xcd_item(blockIdx.x, gridDim.x, a.xcd_map), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t s0 = a.bstart[b], n = a.bstart[b + 1] - s0;
    if (n > kBucketCap || n == 0) {  // (too big: flagged by k_part_starts, the caller falls back to the general path)
        if (tid == 0) a.ucount[b] = 0;
        return;
    }
    const int sub_bits = a.low_bits < kSubBits ? a.low_bits : kSubBits;   // sub-bucket = top sub_bits of hash_low
    const int sub_shift = a.gb + a.low_bits - sub_bits;                   // sort key = hash_low << gb | genome
    const uint32_t n_sub = 1u << sub_bits;
    const uint32_t gmask = (1u << a.gb) - 1u, rmask = (1u << a.rb) - 1u;

    for (uint32_t s = tid; s < n_sub; s += T) sb_cur[s] = 0;
    K key[EPT];
    uint32_t dst[EPT];  // where the element's slice record goes (the fast path takes H < 2^30): requested now, used after the sort
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        const uint32_t k = tid + j * T;
        key[j] = (K)~(K)0;
        dst[j] = 0;
        if (k < n) {
            const unsigned long long full = a.keys[s0 + k];
            // (the partition ran in the caller's genome order while the internal order was still being computed: the
            // genome field is translated here, one gather from an L2-resident table)
            const uint32_t gc = (uint32_t)(full >> a.rb) & gmask;
            uint32_t gi = gc, row0;
            if (a.tab) {
                const uint2 t = a.tab[gc];
                gi = t.x;
                row0 = t.y;
            } else {
                row0 = (uint32_t)a.off_new[gc];
            }
            key[j] = (K)(((full >> (a.rb + a.gb)) << a.gb) | gi);
            dst[j] = row0 + ((uint32_t)full & rmask);
        }
    }
    __syncthreads();
    if (a.debug & 8) { if (key[0] == 12345 && dst[0] == 77) a.ucount[b] = 1; return; }
    // counting sort by sub-bucket: ONE atomic per key -- it also tells the key's place inside its sub-bucket
    uint32_t rank[EPT];
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        rank[j] = 0;
        if (tid + j * T < n) rank[j] = atomicAdd(&sb_cur[(uint32_t)(key[j] >> sub_shift)], 1u);
    }
    __syncthreads();
    {   // exclusive scan of the sub-bucket counts: kSub / T consecutive entries per thread
        constexpr uint32_t PER = (kSub + T - 1) / T;
        uint32_t v[PER], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < PER; i++) {
            const uint32_t s = tid * PER + i;
            v[i] = s < n_sub ? sb_cur[s] : 0u;
            sum += v[i];
        }
        uint32_t incl = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if ((int)lane >= o) incl += t;
        }
        if (lane == 63) wave_part[wave] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t w = 0; w < wave; w++) run += wave_part[w];
#pragma unroll
        for (uint32_t i = 0; i < PER; i++) {
            const uint32_t s = tid * PER + i;
            if (s < n_sub) sb_start[s] = run;
            run += v[i];
        }
        if (tid == 0) sb_start[n_sub] = n;
        __syncthreads();
    }
    constexpr uint32_t VPER = 16 / sizeof(K);   // keys per 16-byte LDS read
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++)
        if (tid + j * T < n) S[sb_start[(uint32_t)(key[j] >> sub_shift)] + rank[j]] = key[j];
    if (tid < VPER && n + tid < kBucketCap) S[n + tid] = (K)~(K)0;   // (the ranking below reads whole 16-byte groups)
    __syncthreads();
    if (a.debug & 16) { if (S[tid] == 12345 && dst[0] == 77) a.ucount[b] = 1; return; }
    // rank = number of smaller keys (keys are distinct: a genome holds a hash once).  The keys of earlier sub-buckets are
    // smaller, those of later ones (and the padding) bigger, so a thread may compare with whole aligned groups of VPER keys
    // around its sub-bucket: one LDS read per group -- a clade-wide hash (a sub-bucket of 10-20 keys) costs its lanes 3-5
    // steps instead of 10-20, and with them every wave that holds one.
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        rank[j] = 0;
        if (tid + j * T < n) {
            const uint32_t s = (uint32_t)(key[j] >> sub_shift);
            const uint32_t q0 = sb_start[s] & ~(VPER - 1), hi = sb_start[s + 1];
            uint32_t r = q0;
            for (uint32_t q = q0; q < hi; q += VPER) {
                if constexpr (sizeof(K) == 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(&S[q]);
                    r += (uint32_t)(v.x < key[j]) + (uint32_t)(v.y < key[j]) + (uint32_t)(v.z < key[j]) + (uint32_t)(v.w < key[j]);
                } else {
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(&S[q]);
                    r += (uint32_t)(v.x < key[j]) + (uint32_t)(v.y < key[j]);
                }
            }
            rank[j] = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++)
        if (tid + j * T < n) S[rank[j]] = key[j];
    __syncthreads();
    if (a.debug & 32) { if (S[tid] == 12345 && dst[0] == 77) a.ucount[b] = 1; return; }
    // (the list masks of the emission below live in the upper half of S -- buckets of at most kBucketCap / 2 keys, nearly all --;
    // zeroed here, the barriers of the head numbering stand between this and their use)
    const bool list_masks = n <= kBucketCap / 2 && !(a.debug & 64);
    uint32_t *lmask = reinterpret_cast<uint32_t *>(&S[kBucketCap / 2]);
    if (list_masks)
        for (uint32_t gi = tid; gi < n; gi += T) lmask[gi] = 0;

    // ---- the bucket is sorted by (hash, genome): S[0 .. n).  List heads are numbered by a scan over contiguous
    // stretches (one per thread); gidx[k] = list of position k
    const uint32_t per = (n + T - 1) / T;
    const uint32_t k0 = min(n, tid * per), k1 = min(n, k0 + per);
    auto is_head = [&](uint32_t k) { return k == 0 || (S[k] >> a.gb) != (S[k - 1] >> a.gb); };
    uint32_t mine = 0;
    for (uint32_t k = k0; k < k1; k++) mine += is_head(k);
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if ((int)lane >= o) incl += t;
    }
    if (lane == 63) wave_part[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, U = 0;
    for (uint32_t w = 0; w < NW; w++) {
        if (w < wave) before += wave_part[w];
        U += wave_part[w];
    }
    {
        uint32_t at = before;  // heads before k0
        for (uint32_t k = k0; k < k1; k++) {
            if (is_head(k)) hd[at++] = (uint16_t)k;
            gidx[k] = (uint16_t)(at - 1);
        }
        if (tid == 0) hd[U] = (uint16_t)n;   // (n <= 4,096 fits)
    }
    __syncthreads();
    if (tid == 0) a.ucount[b] = U;
    if (a.debug & 4) return;

    // ---- postings and list heads in sorted order (coalesced stores)
    if (!(a.debug & 2)) {
        for (uint32_t k = tid; k < n; k += T) a.postings[s0 + k] = (uint32_t)S[k] & gmask;
        const unsigned long long hash_hi = (unsigned long long)b << a.low_bits;
        for (uint32_t gi = tid; gi < U; gi += T) {
            const uint32_t k = hd[gi];
            const unsigned long long hh = hash_hi | (unsigned long long)(S[k] >> a.gb);
            if (a.tmp_uhash64) a.tmp_uhash64[s0 + gi] = hh;
            else a.tmp_uhash[s0 + gi] = (uint32_t)hh;
            a.tmp_upos[s0 + gi] = s0 + k;
        }
    }
    // ---- (round 4) the genomes of every list as ONE bit mask relative to the list's first genome, gathered with one LDS
    // atomic per element (instead of every element walking the rest of its list: in a wave the longest list set the pace).
    // The masks live in the upper half of S, so only in buckets of at most kBucketCap / 2 keys (nearly all); lists that
    // span more than 32 ids keep the walk.
    if (list_masks) {
#pragma unroll
        for (uint32_t j = 0; j < EPT; j++) {
            if (tid + j * T >= n) continue;
            const uint32_t gi = gidx[rank[j]];
            const uint32_t gs = hd[gi];
            const uint32_t d = ((uint32_t)key[j] & gmask) - ((uint32_t)S[gs] & gmask);
            if (d < 32u && hd[gi + 1] - gs > 1u) atomicOr(&lmask[gi], 1u << d);
        }
        __syncthreads();
    }
    // ---- slice records, every element by the thread that loaded it
    uint32_t n_flagged = 0;
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        if (tid + j * T >= n) continue;
        const uint32_t k = rank[j];
        const uint32_t gi = gidx[k];
        const uint32_t gs = hd[gi], ge = hd[gi + 1];
        const uint32_t g = (uint32_t)key[j] & gmask;
        uint2 rec = make_uint2(0, 0);
        if (k + 1 < ge) {
            const uint32_t first = (uint32_t)S[k + 1] & gmask, last = (uint32_t)S[ge - 1] & gmask;
            // covered (row pairs): the odd genome's predecessor in the list is its pair partner
            const bool covered = (g & 1u) && k > gs && ((uint32_t)S[k - 1] & gmask) == g - 1;
            if (last - first <= 31u) {
                uint32_t mask = 0;
                const uint32_t g0 = (uint32_t)S[gs] & gmask;
                if (list_masks && last - g0 <= 31u) mask = lmask[gi] >> (first - g0);
                else
                    for (uint32_t m = k + 1; m < ge; m++) mask |= 1u << (((uint32_t)S[m] & gmask) - first);
                rec = make_uint2(0x80000000u | first, covered ? mask & ~1u : mask);
            } else {
                const uint32_t near_flag = first - g <= 32u ? 0x80000000u : 0u;
                n_flagged += near_flag >> 31;
                rec = make_uint2((s0 + k + 1) | (covered ? 0x40000000u : 0u), (s0 + ge) | near_flag);
            }
        }
        if (!(a.debug & 1)) a.self_raw[dst[j]] = rec;
    }
    // related lists wider than a compact record, counted in every 16th bucket (a uniform sample of the hashes; same-address
    // atomics cost ~13 ns each, so not one per workgroup): tells the self join whether the collection has clusters wider
    // than the 32-column window of rk_near_kernel
    if ((b & 15u) == 0) {
        for (int o = 32; o > 0; o >>= 1) n_flagged += __shfl_down(n_flagged, o);
        if (lane == 0 && n_flagged) atomicAdd(&a.res->flagged, 16ULL * n_flagged);
    }
}

// single workgroup: ubase = exclusive scan of the buckets' list counts; U
// (several passes: the lists of this pass go behind those of the passes before, res->U so far)
__global__ void k_heads_scan(const uint32_t *ucount, uint32_t nb, uint32_t *ubase, BuildResult *res)
{
    const uint32_t u0 = (uint32_t)res->U;
    __syncthreads();
    const uint32_t all = block_scan_sweeps<uint32_t>(nb, [&](uint32_t b) { return ucount[b]; },
                                                     [&](uint32_t b, uint32_t before) { ubase[b] = u0 + before; });
    if (threadIdx.x == 0) {
        ubase[nb] = u0 + all;
        res->U = (unsigned long long)u0 + all;
    }
}

// one workgroup per bucket: its list heads move to their place among all distinct hashes
// (pass_base: postings written by the passes before this one -- the temporaries are indexed by global posting position)
template <class HT>
__global__ void k_heads_place(const HT *tmp_uhash, const uint32_t *tmp_upos, const uint32_t *bstart, const uint32_t *ucount,
                              const uint32_t *ubase, uint32_t nb, const unsigned long long *pass_base, HT *uhash, uint32_t *upos)
{
    const uint32_t b = blockIdx.x;
    const uint32_t s0 = (uint32_t)pass_base[0] + bstart[b], n = ucount[b], d0 = ubase[b];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        uhash[d0 + i] = tmp_uhash[s0 + i];
        upos[d0 + i] = tmp_upos[s0 + i];
    }
    if (b == nb - 1 && threadIdx.x == 0) upos[ubase[nb]] = (uint32_t)pass_base[1];   // (the end of the last list so far)
}

// one wave per genome: number of open / covered slices of its row (class carried by the record, slice_class2)
__global__ void k_row_counts2(const uint64_t *off, uint32_t n_genomes, const uint2 *self_raw, uint32_t *n_open, uint32_t *n_cov)
{
    const uint32_t g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_genomes) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t e1 = off[g + 1];
    uint32_t no = 0, nc = 0;
    for (uint64_t e = off[g] + lane; e < e1; e += 64) {
        const uint8_t c = slice_class2(self_raw[e]);
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

// one wave per genome: open slices to the front of the row, covered ones behind them, empty ones dropped
__global__ void k_row_place2(const uint64_t *off, uint32_t n_genomes, const uint2 *self_raw, const uint64_t *self_off,
                             const uint64_t *self_split, uint2 *out)
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
        const uint8_t c = slice_class2(raw);
        const uint2 r = slice_final2(raw);
        const unsigned long long mo = __ballot(c == kOpen), mc = __ballot(c == kCovered);
        if (c == kOpen) out[at_open + __popcll(mo & lt)] = r;
        if (c == kCovered) out[at_cov + __popcll(mc & lt)] = r;
        at_open += __popcll(mo);
        at_cov += __popcll(mc);
    }
}
