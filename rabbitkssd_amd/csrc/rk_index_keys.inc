// rk_index_keys.inc -- a sharded build from PER-RANK sketches (included by rk_index.hip inside its anonymous namespace, behind
// rk_index_fast.inc).
//
// rk_index_build_shard assumes that every shard holds the whole collection.  A collection sketched on N ranks is not held that
// way: rank r has the sketches of its own genomes only.  Here every rank cuts its sketches into 8-byte keys by destination shard
// (the hash range a key belongs to), ONE all-to-all moves them, and every shard builds its posting lists from the keys that
// arrived; the renumbering needs only the 16 smallest hashes and the size of every genome (an all-gather of 68 bytes per genome).
//
//   k_sketch_signature  per genome: size, then its min(16, size) smallest hashes folded to 32 bits (fold_hash), zero-padded
//   k_sketch_split      <kWrite = false> keys per destination shard; <kWrite = true> the keys themselves, contiguous by destination
//   k_split_bases       one thread: where each destination's keys start in the send buffer
//   k_keys_pass_filter  (a shard in several passes) the keys of one pass, re-based to the bits inside the pass
//   k_sig_sizes         the sizes of the all-gathered signatures and their sum, largest and smallest (the renumbering reads the
//                       signatures themselves: SigMinK)
//
// Wire format of a key (include/rabbitkssd.h): (hash with its top shard_bits removed) << gb | global genome id -- the layout
// k_range_filter writes for the range passes (FastArgs.filtered), so the received keys ARE a filtered partition source.
// HBM-bound streaming; integer arithmetic, no MFMA.

constexpr uint32_t kSigWords = RK_SIG_WORDS;   // size + kMinK hashes

template <class K>
__global__ void k_sketch_signature(const K *hashes, const uint64_t *off, uint32_t n, uint32_t *sig)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint64_t e0 = off[g], sz = off[g + 1] - e0;
    uint32_t *o = sig + (size_t)g * kSigWords;
    o[0] = (uint32_t)sz;
#pragma unroll
    for (uint32_t i = 0; i < kMinK; i++) o[1 + i] = i < sz ? fold_hash(hashes[e0 + i]) : 0u;
}

struct SplitArgs {
    const void *hashes;          // the rank's CSR: u32, or u64 (64-bit hash layout)
    const uint64_t *off;
    uint64_t H;                  // the rank's elements
    uint32_t n_local, genome_base;
    int hash_bits, shift, gb;    // destination = hash >> shift (n_dest > 1); key = (hash & rem_mask) << gb | genome_base + local genome
    unsigned long long rem_mask;
    uint32_t n_dest;
    int xcd_map;
};

// As k_range_filter: four workgroups of 256 threads per chunk of kPartChunk elements, every wave a stretch of 64 steps of 64 lanes
// (the walk reads the stretch again, from the cache: held in registers, 64 hashes per lane took 256 VGPRs -- or scratch -- beside the
// loop over destinations).  A rank's sketches are sorted inside every genome, so the 64
// hashes of a step fall into one or two destinations: a step costs one ballot per destination it touches, and the keys of a
// destination leave as one contiguous run.  Counting: per wave and destination in LDS, then ONE atomic per (workgroup,
// destination) -- on the destination's count (kWrite = false) or on its cursor in the send buffer (kWrite = true).
constexpr uint32_t kSplitThreads = 256, kSplitPerChunk = 4;
template <class HT, bool kWrite>
__global__ __launch_bounds__(kSplitThreads) void k_sketch_split(SplitArgs a, const uint32_t *chunk_first, unsigned long long *dest,
                                                               unsigned long long *out, unsigned int *bad)
{
    constexpr uint32_t nw = kSplitThreads / 64;
    constexpr uint32_t kSteps = kPartChunk / (64 * nw * kSplitPerChunk);
    __shared__ uint64_t stage[kStageGenomes];
    __shared__ uint32_t wcnt[nw][kRecRegions];
    __shared__ unsigned long long wbase[nw][kRecRegions];
    const HT *hashes = static_cast<const HT *>(a.hashes);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t item = xcd_item(blockIdx.x, gridDim.x, a.xcd_map);
    const uint32_t chunk = item / kSplitPerChunk, part = item % kSplitPerChunk;
    const uint64_t c0 = (uint64_t)chunk * kPartChunk, c1 = min(a.H, c0 + kPartChunk);
    const uint64_t w0 = min(c1, c0 + (uint64_t)(part * nw + wave) * (64 * kSteps)), w1 = min(c1, w0 + 64 * kSteps);
    wcnt[wave][lane] = 0;   // (kRecRegions == 64: one entry per lane)
    uint32_t ga = 0, gb = 0;
    bool staged = false;
    if (kWrite) {
        ga = chunk_first[chunk];
        gb = chunk_first[chunk + 1];
        staged = gb - ga + 1 <= kStageGenomes;
        if (staged)
            for (uint32_t k = tid; k <= gb - ga; k += kSplitThreads) stage[k] = a.off[ga + k + 1];
    }
    __syncthreads();
    auto outside = [&](HT h) { return a.hash_bits < (int)(8 * sizeof(HT)) && (h >> a.hash_bits) != 0; };
    auto dest_of = [&](HT h) { return a.n_dest > 1 ? (uint32_t)((unsigned long long)h >> a.shift) : 0u; };
    bool saw_bad = false;
    // (all lanes arrive: the loop over the destinations of a step is wave-uniform.  The count of the destination the wave is in
    // stays in a register while the run lasts -- consecutive steps mostly stay in one -- and goes to LDS when the run ends)
    uint32_t run_d = 0, run_n = 0;
    auto count_step = [&](bool valid, HT h) {
        const bool ok = valid && !outside(h);
        saw_bad |= valid && !ok;
        const uint32_t d = ok ? dest_of(h) : 0u;
        unsigned long long pending = __ballot(ok);
        while (pending) {
            const uint32_t dl = (uint32_t)__shfl((int)d, __ffsll((long long)pending) - 1);
            const unsigned long long m = __ballot(ok && d == dl);
            if (dl != run_d) {
                if (run_n) wcnt[wave][run_d] = wcnt[wave][run_d] + run_n;   // (every lane writes the same value)
                run_d = dl;
                run_n = 0;
            }
            run_n += (uint32_t)__popcll(m);
            pending &= ~m;
        }
    };
    for (uint64_t e = w0 + lane; e - lane < w1; e += 64) count_step(e < w1, e < w1 ? hashes[e] : (HT)0);
    if (run_n) wcnt[wave][run_d] = wcnt[wave][run_d] + run_n;
    if (!kWrite && saw_bad && bad) atomicOr(bad, 1u);
    __syncthreads();
    if (tid < a.n_dest) {
        unsigned long long all = 0;
        for (uint32_t w = 0; w < nw; w++) all += wcnt[w][tid];
        if (!kWrite) {
            if (all) atomicAdd(&dest[tid], all);
        } else {
            unsigned long long at = all ? atomicAdd(&dest[tid], all) : 0ULL;
            for (uint32_t w = 0; w < nw; w++) {
                wbase[w][tid] = at;
                at += wcnt[w][tid];
            }
        }
    }
    if (!kWrite) return;
    __syncthreads();
    if (w0 >= w1) return;
    auto end_of = [&](uint32_t i) -> uint64_t { return staged ? stage[i - ga] : a.off[i + 1]; };
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
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    uint32_t cur_d = 0;
    unsigned long long cur = wbase[wave][0];   // (the cursor of the destination the wave writes to, kept in a register while the run lasts)
    auto write_step = [&](uint64_t e, bool valid, HT h) {
        const bool ok = valid && !outside(h);
        if (ok)
            while (e >= i_end) {   // next genome (empty sketches are stepped over)
                i++;
                i_end = end_of(i);
            }
        const uint32_t d = ok ? dest_of(h) : 0u;
        const unsigned long long key = (((unsigned long long)h & a.rem_mask) << a.gb) | (unsigned long long)(a.genome_base + i);
        unsigned long long pending = __ballot(ok);
        while (pending) {
            const uint32_t dl = (uint32_t)__shfl((int)d, __ffsll((long long)pending) - 1);
            const bool mine = ok && d == dl;
            const unsigned long long m = __ballot(mine);
            if (dl != cur_d) {
                wbase[wave][cur_d] = cur;   // (every lane writes the same value)
                cur_d = dl;
                cur = wbase[wave][dl];
            }
            if (mine) out[cur + (uint32_t)__popcll(m & lt)] = key;
            cur += (uint32_t)__popcll(m);
            pending &= ~m;
        }
    };
    for (uint64_t e = w0 + lane; e - lane < w1; e += 64) write_step(e, e < w1, e < w1 ? hashes[e] : (HT)0);   // (read again: from the cache)
}

// counts[0 .. n_dest) -> cursors[d] = keys of the destinations before d (where its keys start in the send buffer)
__global__ void k_split_bases(const unsigned long long *counts, uint32_t n_dest, unsigned long long *cursors)
{
    if (threadIdx.x != 0) return;
    unsigned long long at = 0;
    for (uint32_t d = 0; d < n_dest; d++) {
        cursors[d] = at;
        at += counts[d];
    }
}

// One pass of a shard that is built in several: the received keys whose hash bits (rem_bits of them) start with `pass`, their
// hash cut to the bits inside the pass.  As k_range_filter: count per wave, ONE reservation per workgroup, every step of 64 lanes
// written as one contiguous run.  A key with hash bits beyond rem_bits is outside the wire format: it raises kFastBadHash (the
// build is refused, as k_part_hist refuses it in a single pass), it is never cut down to a valid key.
constexpr uint32_t kKeysFilterThreads = 256, kKeysFilterSteps = 16;
__global__ __launch_bounds__(kKeysFilterThreads) void k_keys_pass_filter(const unsigned long long *in, uint64_t n, int gb, int rem_bits, int pass_bits,
                                                                         uint32_t pass, unsigned long long *out, unsigned long long *cursor,
                                                                         unsigned long long cap, BuildResult *res)
{
    constexpr uint32_t nw = kKeysFilterThreads / 64;
    __shared__ uint32_t wave_cnt[nw];
    __shared__ unsigned long long s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t w0 = ((uint64_t)blockIdx.x * nw + wave) * (64 * kKeysFilterSteps);
    const int in_bits = rem_bits - pass_bits;   // hash bits inside the pass
    unsigned long long kv[kKeysFilterSteps];
    uint32_t cnt = 0;
    auto keep = [&](unsigned long long k) { return ((k >> gb) >> in_bits) == (unsigned long long)pass; };
    bool bad = false;
#pragma unroll
    for (uint32_t j = 0; j < kKeysFilterSteps; j++) {
        const uint64_t e = w0 + 64 * j + lane;
        kv[j] = e < n ? in[e] : 0ULL;
        cnt += e < n && keep(kv[j]);
        bad |= e < n && ((kv[j] >> gb) >> rem_bits) != 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
    if (lane == 0) wave_cnt[wave] = cnt;
    if (__ballot(bad) && lane == 0) atomicOr(&res->flags, (unsigned long long)kFastBadHash);
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < nw; w++) all += wave_cnt[w];
        unsigned long long at = all ? atomicAdd(cursor, (unsigned long long)all) : 0ULL;
        if (at + all > cap) {   // (cannot happen: the pass's buffer holds all of the shard's keys)
            atomicOr(&res->flags, kFastOverflow);
            at = ~0ULL;
        }
        s_base = at;
    }
    __syncthreads();
    if (s_base == ~0ULL || cnt == 0) return;   // (cnt: the wave's sum, uniform)
    unsigned long long at = s_base;
    for (uint32_t w = 0; w < wave; w++) at += wave_cnt[w];
    const unsigned long long lt = (1ULL << lane) - 1ULL, gmask = (1ULL << gb) - 1ULL, hmask = (1ULL << in_bits) - 1ULL;
#pragma unroll
    for (uint32_t j = 0; j < kKeysFilterSteps; j++) {
        const uint64_t e = w0 + 64 * j + lane;
        const bool k = e < n && keep(kv[j]);
        const unsigned long long m = __ballot(k);
        if (k) out[at + (uint32_t)__popcll(m & lt)] = (((kv[j] >> gb) & hmask) << gb) | (kv[j] & gmask);
        at += (uint32_t)__popcll(m);
    }
}

// the partition source of a single-pass shard: the received keys themselves, n of them
__global__ void k_set_u64(unsigned long long *p, unsigned long long v)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *p = v;
}

// signatures (global order) -> sizes, and their statistics: stats[0] = sum of the sizes, stats[1] = the largest, stats[2] = the smallest
// non-zero one (0xFFFFFFFF: none; stats arrive as {0, 0, ~0}).  A grid of at most kSigSizesBlocks workgroups strides over the genomes
// and every workgroup reduces in LDS before its three atomics (one per wave: 23,000 atomics on three words took 0.28 ms at 500,000
// genomes).
constexpr uint32_t kSigSizesBlocks = 256, kSigSizesThreads = 1024;
__global__ __launch_bounds__(kSigSizesThreads) void k_sig_sizes(const uint32_t *sig, uint32_t n, uint32_t *sizes, unsigned long long *stats)
{
    __shared__ unsigned long long s_tot[kSigSizesThreads / 64];
    __shared__ uint32_t s_mx[kSigSizesThreads / 64], s_mn[kSigSizesThreads / 64];
    unsigned long long tot = 0;
    uint32_t mx = 0, mn = 0xFFFFFFFFu;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
        const uint32_t sz = sig[(size_t)g * kSigWords];
        sizes[g] = sz;
        tot += sz;
        mx = max(mx, sz);
        if (sz) mn = min(mn, sz);
    }
    for (int o = 32; o > 0; o >>= 1) {
        tot += __shfl_xor(tot, o);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_tot[wave] = tot;
        s_mx[wave] = mx;
        s_mn[wave] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kSigSizesThreads / 64; w++) {
            tot += s_tot[w];
            mx = max(mx, s_mx[w]);
            mn = min(mn, s_mn[w]);
        }
        atomicAdd(&stats[0], tot);
        atomicMax(&stats[1], (unsigned long long)mx);
        atomicMin(&stats[2], (unsigned long long)mn);
    }
}
