// rk_index_tiles.inc -- the tile records of the self join (rk_dist_tile.inc) as a PRODUCT OF THE INDEX BUILD (round 5;
// included by rk_index.hip behind rk_index_fast.inc, inside its anonymous namespace).
//
// Until round 4 the fast build emitted one slice record per (genome, hash) element -- the input of rk_near_kernel -- and the
// tile records were derived lazily from the finished postings by a chain of device-wide scans and sorts (rk_tiles.hip:
// 1.2 ms warm, 19-34 ms with its code objects): the first join over an index never ran on the tile kernel.  Here the
// bucket emission writes tile records instead of slice records while a bucket's lists are still in LDS, and six small
// kernels sort them by tile and write the directory:
//
//   k_bucket_emit_tiles  as k_bucket_emit up to the sorted bucket; then per "run" (the members of one list inside one block
//                        of 32 genome ids) one record per earlier run of its list -- tile (block_i, block_j), (mask_i, mask_j) --
//                        and one for itself when it holds two members; records leave unsorted, 64 regions with a cursor each
//   k_trec_count         records per ROW block b (LDS histogram per workgroup, one global atomic per non-empty bin)
//   k_trec_starts        one workgroup: bin starts, and the order in which the row sort takes the row blocks (the fullest first)
//   k_trec_scatter       records to their row block's bin (a workgroup reserves one run per bin)
//   k_trec_rowsort       workgroups draw row blocks from that list: a block's records by column block w (LDS counting sort, one
//                        LDS word per column block), every tile from an EVEN slot of the final arrays (AoS + the split copy of the
//                        scalar-row kernel variant); per tile a proto directory entry with its density level for both metrics
//   k_tdir_scan          one workgroup: tiles per level -> level starts, the host's prefix table
//   k_tdir_place         the directory in launch order (level by level, densest first), one 32-byte entry per tile and metric;
//                        a workgroup per eight row blocks
//
// No rocprim, nothing lazy, one read-back (with the build's own).  The unsorted records have a fixed capacity (H / 2 + 64 K:
// clades of ten need 0.15 H, species of 1,000 strains 0.29 H); a collection whose lists scatter over many blocks overflows
// it -- the kernels raise a flag and stand still, and the host builds the index with slice records instead.
// Integer / LDS work, HBM-bound streaming; no MFMA.

constexpr uint32_t kRecRegions = 64;     // cursors of the unsorted records (one per workgroup would be 8,192 same-address atomics)
constexpr uint32_t kRecParts = 8;        // workgroups per region in the counting / scattering passes
constexpr uint32_t kCrowdedSub = 768;     // keys in one sub-bucket of the LDS counting sort from which a bucket is left to k_bucket_heavy
constexpr uint32_t kTileMaxBlocks = 16384;  // row sort: two LDS words per column block (524,288 genomes)

struct TileResult {   // written by the kernels, read back once with the BuildResult
    unsigned long long overflow;        // the unsorted records did not fit: nothing below is meaningful
    unsigned long long n_records, n_slots, n_tiles, max_records;
    unsigned long long level_count[2][kTileTable + 1];   // tiles per (metric, level); k_tdir_scan turns it into "tiles of this level or denser"
    unsigned long long rec_count[kRecRegions];   // records ASKED for per region (beyond its capacity: overflow)
};
struct TileCursors {  // zeroed with the partition's cursors
    unsigned long long final_at, tile_at;        // slots / proto entries handed out by k_trec_rowsort
    unsigned long long ticket;                   // the next row block of the row sort's list
    unsigned long long level_at[2][kTileTable + 1];
};

struct TileEmitArgs {
    const unsigned long long *keys;   // the partition's keys: hash_low << (gb + rb) | caller's genome << rb | position (rb = 0 here)
    const uint32_t *bstart;
    const uint32_t *inv;              // caller's genome index -> internal id (null: identity)
    int low_bits, gb, rb;
    uint32_t nb;
    uint32_t *postings;
    uint32_t *tmp_uhash, *tmp_upos;
    unsigned long long *tmp_uhash64;
    uint32_t *ucount;
    uint3 *rec;                       // (row block << 16 | column block, row mask, column mask): one 12-byte store
    uint32_t region_cap;
    // (round 5, sharded / multi-pass builds) this pass covers one range of the hash space: its postings go behind those of the
    // passes before (pass_base[0], on the device), hash_base = the range's first hash; n_dest > 1: the records are grouped by the
    // shard that owns their ROW block (blocks of 32 genomes dealt round-robin: block % n_dest), kRecRegions / n_dest regions each
    const unsigned long long *pass_base;
    unsigned long long hash_base;
    uint32_t n_dest;
    const BuildResult *stop;          // range passes: a pass with more keys than the key buffers hold raised a flag -- stand still
    int big_ok;                       // buckets of more than kBucketCap keys are listed by k_part_starts and built by k_bucket_heavy
    BuildResult *stop_rw;             // (k_bucket_heavy raises the overflow flag for what it cannot take)
    uint32_t *big_list, *n_big;       // the pass's list of buckets for k_bucket_heavy (k_part_starts starts it, the emission adds the crowded ones)
    TileResult *tres;
    int xcd_map;
    int debug;   // developer ablations (RK_INDEX_DEBUG; the index is then wrong by design): 8 stop after the load, 16 after the counting sort, 32 after the rank sort, 4 after the numbering, 2 no posting / head stores, 1 no tile records, 64 the slabs of k_bucket_heavy stay unsorted
};

// smallest k with n / lb >= 2^(-k/8) (less the margin of the host's table, rk_dist_tile.inc tile_launch_shape); kTileTable: none
__device__ inline uint32_t tile_level(uint32_t n, uint32_t lb)
{
    const float ratio = (float)n / (float)lb;
    if (!(ratio > 0.0f)) return kTileTable;
    auto theta = [](int k) { return exp2f(-(float)k / 8.0f) * (1.0f - 1e-4f); };
    const float kf = ceilf(-8.0f * log2f(ratio));
    int k = kf < 0.0f ? 0 : (kf > (float)kTileTable ? kTileTable : (int)kf);
    while (k > 0 && ratio >= theta(k - 1)) k--;
    while (k < kTileTable && !(ratio >= theta(k))) k++;
    return (uint32_t)k;
}

// What leaves a SORTED stretch of a bucket -- S[0 .. n) ascending by (hash_low << gb | internal genome) --: postings at
// post_base + k, list heads at head_base + (list number), tile records.  Shared by k_bucket_emit_tiles (the whole bucket) and
// k_bucket_heavy (a slab of a bucket beyond the LDS sort).  write_ucount: the stretch is the whole bucket.  Returns the
// stretch's number of lists (uniform).
template <int T, class K>
__device__ inline uint32_t emit_sorted_bucket(const TileEmitArgs &a, const K *S, uint16_t *hd, uint16_t *rpos, uint32_t *wave_part, uint32_t *s_cnt,
                                              uint32_t *s_cur, unsigned long long *s_dbase, uint32_t n, uint32_t b, uint32_t post_base, uint32_t head_base,
                                              unsigned long long hash_hi, bool write_ucount, uint32_t *rmask)
{
    constexpr uint32_t NW = T / 64, EPT = kBucketCap / T;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t gmask = (1u << a.gb) - 1u;
    // ---- the bucket is sorted by (hash, genome): S[0 .. n).  List heads AND runs (a list's members inside one block of 32
    // ids) are numbered by ONE scan over contiguous stretches: heads in the low half of the packed count, runs in the high half.
    // A thread reads its stretch (at most EPT keys and the one before) ONCE, into registers; the flags are two bit masks.
    const uint32_t per = (n + T - 1) / T;   // <= EPT
    const uint32_t k0 = min(n, tid * per), k1 = min(n, k0 + per);
    auto genome = [&](uint32_t k) { return (uint32_t)S[k] & gmask; };
    uint32_t head_bits = 0, run_bits = 0;
    {
        K prev = k0 ? S[k0 - 1] : (K)0;
#pragma unroll
        for (uint32_t i = 0; i < EPT; i++) {
            const uint32_t k = k0 + i;
            if (i < per && k < k1) {   // (i < per: uniform)
                const K cur = S[k];
                const bool head = k == 0 || (cur >> a.gb) != (prev >> a.gb);
                const bool run = head || (((uint32_t)cur & gmask) >> 5) != (((uint32_t)prev & gmask) >> 5);
                head_bits |= (head ? 1u : 0u) << i;
                run_bits |= (run ? 1u : 0u) << i;
                prev = cur;
            }
        }
    }
    const uint32_t mine = (uint32_t)__popc(head_bits) + ((uint32_t)__popc(run_bits) << 16);
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if ((int)lane >= o) incl += t;
    }
    if (lane == 63) wave_part[wave] = incl;
    __syncthreads();   // (also: every thread is done with sb_start -- rpos overlays it)
    uint32_t before = incl - mine, all = 0;
    for (uint32_t w = 0; w < NW; w++) {
        if (w < wave) before += wave_part[w];
        all += wave_part[w];
    }
    const uint32_t U = all & 0xFFFFu, R = all >> 16;
    {
        uint32_t at_h = before & 0xFFFFu, at_r = before >> 16;
#pragma unroll
        for (uint32_t i = 0; i < EPT; i++) {
            if (i >= per) break;   // (uniform)
            const uint32_t k = k0 + i;
            const bool head = (head_bits >> i) & 1u;
            if (head) hd[at_h++] = (uint16_t)k;
            if ((run_bits >> i) & 1u) rpos[at_r++] = (uint16_t)(k | (head ? 0x8000u : 0u));   // (bit 15: the first run of its list; k <= 4,096)
        }
        if (tid == 0) {
            hd[U] = (uint16_t)n;
            rpos[R] = (uint16_t)(n | 0x8000u);
        }
    }
    __syncthreads();
    if (tid == 0 && write_ucount) a.ucount[b] = U;
    if (a.debug & 4) return U;

    // ---- tile records: run j pairs with every earlier run i of its list -- tile (block_i, block_j), (mask_i, mask_j) -- and
    // with itself when it holds two members.  One run per thread and round (a bucket holds ~0.3 runs per key: one round);
    // masks are gathered by walking the run (at most 32 members); a list's first run carries a flag, so "the earlier runs of
    // my list" is a walk back to it.  The round's records are counted first; their place in the region comes from ONE
    // returning device-scope atomic per workgroup, whose round trip (~2 us) hides behind the posting and list-head stores.
    auto run_at = [&](uint32_t r) { return (uint32_t)rpos[r] & 0x7FFFu; };
    auto walk_mask = [&](uint32_t r) {
        uint32_t m = 0;
        for (uint32_t k = run_at(r), e = run_at(r + 1); k < e; k++) m |= 1u << (genome(k) & 31u);
        return m;
    };
    // (rmask: room for one mask per run, when the caller has it -- a list of a whole species has dozens of runs, and every pair of
    // them names two masks: walked per pair that was 40 us per such list)
    if (rmask) {
        for (uint32_t r = tid; r < R; r += T) rmask[r] = walk_mask(r);
        __syncthreads();
    }
    auto run_mask = [&](uint32_t r) { return rmask ? rmask[r] : walk_mask(r); };
    const uint32_t n_dest = a.n_dest, n_sub_regions = kRecRegions / n_dest;
    auto dest_of = [&](uint32_t row_block) { return n_dest > 1 ? row_block % n_dest : 0u; };
    bool outputs_done = false;
    auto outputs = [&]() {   // postings and list heads in sorted order (coalesced stores)
        if (a.debug & 2) return;
        for (uint32_t k = tid; k < n; k += T) a.postings[post_base + k] = genome(k);
        for (uint32_t gi = tid; gi < U; gi += T) {
            const uint32_t k = hd[gi];
            const unsigned long long hh = hash_hi | (unsigned long long)(S[k] >> a.gb);
            if (a.tmp_uhash64) a.tmp_uhash64[head_base + gi] = hh;
            else a.tmp_uhash[head_base + gi] = (uint32_t)hh;
            a.tmp_upos[head_base + gi] = post_base + k;
        }
    };
    // run j's records: how many earlier runs its list has (counted per destination when asked), and whether it pairs with itself (two
    // members: the genomes of a list are distinct, so are the bits of its mask)
    auto count_run = [&](uint32_t j, bool add, uint32_t &earlier, bool &self) {
        earlier = 0;
        for (uint32_t i = j; !(rpos[i] & 0x8000u); i--) {
            earlier++;
            if (add) atomicAdd(&s_cnt[dest_of(genome(run_at(i - 1)) >> 5)], 1u);
        }
        self = run_at(j + 1) - run_at(j) >= 2;
        if (self && add) atomicAdd(&s_cnt[dest_of(genome(run_at(j)) >> 5)], 1u);
    };
    auto place_run = [&](uint32_t j, uint32_t earlier, bool self) {
        const uint32_t mask_j = run_mask(j), wj = genome(run_at(j)) >> 5;
        for (uint32_t i = j; i > j - earlier; i--) {
            const uint32_t bi = genome(run_at(i - 1)) >> 5, d = dest_of(bi);
            const unsigned long long base = s_dbase[d];
            const uint32_t at = atomicAdd(&s_cur[d], 1u);
            if (base != ~0ULL) a.rec[base + at] = make_uint3((bi << 16) | wj, run_mask(i - 1), mask_j);
        }
        if (self) {
            const uint32_t d = dest_of(wj);
            const unsigned long long base = s_dbase[d];
            const uint32_t at = atomicAdd(&s_cur[d], 1u);
            if (base != ~0ULL) a.rec[base + at] = make_uint3((wj << 16) | wj, mask_j, mask_j);
        }
    };
    // the counted records' place: one returning device-scope atomic per destination, all in one wave instruction, looked at behind
    // the posting / list-head stores (called by all threads, between two barriers)
    auto reserve = [&]() {
        uint32_t want = 0;
        unsigned long long got = 0;
        uint32_t region = 0;
        if (tid < n_dest) {
            want = s_cnt[tid];
            s_cnt[tid] = 0;
            s_cur[tid] = 0;
            region = tid * n_sub_regions + b % n_sub_regions;
            if (want) got = atomicAdd(&a.tres->rec_count[region], (unsigned long long)want);
        }
        if (!outputs_done) {
            outputs();
            outputs_done = true;
        }
        if (tid < n_dest) {
            unsigned long long base = ~0ULL;
            if (want) {
                if (got + want <= a.region_cap) base = (unsigned long long)region * a.region_cap + got;
                else a.tres->overflow = 1;
            }
            s_dbase[tid] = base;
        }
    };
    if (R && !(a.debug & 1)) {
        // (a bucket of a crowded hash space -- 500,000 genomes in 28 bits: most lists are two unrelated genomes, every key a run --
        // has more runs than threads: ALL rounds are counted first, so that the bucket still asks for its place once)
        uint32_t earlier = 0;
        bool self = false;
        for (uint32_t r0 = 0; r0 < R; r0 += T)   // (uniform)
            if (r0 + tid < R) count_run(r0 + tid, true, earlier, self);
        __syncthreads();
        reserve();
        __syncthreads();
        for (uint32_t r0 = 0; r0 < R; r0 += T)
            if (r0 + tid < R) {
                if (R > T) count_run(r0 + tid, false, earlier, self);   // (several rounds: what the first loop found is gone)
                place_run(r0 + tid, earlier, self);
            }
    }
    if (!outputs_done) outputs();
    return U;
}

// One workgroup of T threads per bucket, the sort exactly as k_bucket_emit (keys in registers + ONE LDS array, counting sort
// by the next 10 hash bits, rank inside the sub-buckets); what leaves: postings, list heads, tile records.
template <int T, class K>
__global__ __launch_bounds__(T, 8) void k_bucket_emit_tiles(TileEmitArgs a)
{
    constexpr uint32_t NW = T / 64, EPT = kBucketCap / T;
    constexpr uint32_t kSub = 1u << kSubBits;
    static_assert(kSub <= 4 * T, "the sub-bucket scan takes at most four entries per thread");
    __shared__ __attribute__((aligned(16))) K S[kBucketCap];
    __shared__ uint16_t hd[kBucketCap + 2];   // hd[i] = position of the i-th list head, hd[U] = n
    __shared__ __attribute__((aligned(16))) uint32_t sb[2 * kSub + 2];   // sub-bucket starts + cursors while sorting; afterwards the runs
    __shared__ uint32_t wave_part[NW];
    uint32_t *sb_start = sb, *sb_cur = sb + kSub + 1;
    uint16_t *rpos = reinterpret_cast<uint16_t *>(sb);   // rpos[r] = first position of run r (| bit 15: its list's first), rpos[R] = n
    static_assert(sizeof(sb) >= (kBucketCap + 1) * sizeof(uint16_t), "rpos overlays the sub-bucket arrays");
    __shared__ uint32_t s_cnt[kRecRegions], s_cur[kRecRegions];   // records of the round per destination shard: counted, then placed
    __shared__ unsigned long long s_dbase[kRecRegions];
    const uint32_t b = xcd_item(blockIdx.x, gridDim.x, a.xcd_map), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t s0 = a.bstart[b], n = a.bstart[b + 1] - s0;
    if (n > kBucketCap && a.big_ok) return;   // (a bucket beyond the LDS sort: k_bucket_heavy takes it, slab by slab)
    if (n > kBucketCap || n == 0 || (a.stop && a.stop->flags)) {  // (too big: flagged by k_part_starts, the caller falls back to the general path)
        if (tid == 0) a.ucount[b] = 0;
        return;
    }
    const uint32_t pb = (uint32_t)a.pass_base[0];   // postings of the passes before this one
    const int sub_bits = a.low_bits < kSubBits ? a.low_bits : kSubBits;
    const int sub_shift = a.gb + a.low_bits - sub_bits;
    const uint32_t n_sub = 1u << sub_bits;
    const uint32_t gmask = (1u << a.gb) - 1u;

    for (uint32_t s = tid; s < n_sub; s += T) sb_cur[s] = 0;
    if (tid < kRecRegions) s_cnt[tid] = s_cur[tid] = 0;
    // (the partition ran in the caller's genome order, see k_bucket_emit: the genome field is translated here, one gather from an
    // L2-resident table -- whose round trip the counting sort does not wait for: a key's sub-bucket is a function of its hash bits)
    K key[EPT];
    uint32_t gi[EPT];
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        const uint32_t k = tid + j * T;
        key[j] = (K)~(K)0;
        gi[j] = 0;
        if (j * T < n && k < n) {   // (j * T < n: uniform -- a bucket holds ~1,500 keys, five of the eight unrolled turns are skipped by a scalar branch)
            const unsigned long long full = a.keys[s0 + k];
            const uint32_t gc = (uint32_t)(full >> a.rb) & gmask;
            gi[j] = a.inv ? a.inv[gc] : gc;
            key[j] = (K)((full >> (a.rb + a.gb)) << a.gb);
        }
    }
    __syncthreads();
    if (a.debug & 8) { if (key[0] == 12345 && gi[0] == 77) a.ucount[b] = 1; return; }
    uint32_t rank[EPT];
    bool crowded = false;
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        rank[j] = 0;
        if (j * T < n && tid + j * T < n) {
            rank[j] = atomicAdd(&sb_cur[(uint32_t)(key[j] >> sub_shift)], 1u);
            crowded |= rank[j] >= kCrowdedSub;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++)
        if (j * T < n && tid + j * T < n) key[j] |= (K)gi[j];
    // (a sub-bucket of hundreds of keys -- a list shared by a whole species -- makes the rank sort below quadratic for its lanes:
    // such a bucket is appended to the list of k_bucket_heavy, whose bitonic sort does not care)
    if (__syncthreads_or(crowded ? 1 : 0) && a.big_ok) {
        if (tid == 0) a.big_list[atomicAdd(a.n_big, 1u)] = b;
        return;
    }
    {
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
    constexpr uint32_t VPER = 16 / sizeof(K);
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++)
        if (j * T < n && tid + j * T < n) S[sb_start[(uint32_t)(key[j] >> sub_shift)] + rank[j]] = key[j];
    if (tid < VPER && n + tid < kBucketCap) S[n + tid] = (K)~(K)0;
    __syncthreads();
    if (a.debug & 16) { if (S[tid] == 12345) a.ucount[b] = 1; return; }
#pragma unroll
    for (uint32_t j = 0; j < EPT; j++) {
        rank[j] = 0;
        if (j * T < n && tid + j * T < n) {
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
        if (j * T < n && tid + j * T < n) S[rank[j]] = key[j];
    __syncthreads();
    if (a.debug & 32) { if (S[tid] == 12345) a.ucount[b] = 1; return; }

    // (no run-mask cache here: a bucket that reaches this point has no crowded sub-bucket -- its lists are short, few of them have a
    // second run, and a mask is walked where a pair needs it; the cache costs ~5 M vector instructions per build for nothing)
    emit_sorted_bucket<T, K>(a, S, hd, rpos, wave_part, s_cnt, s_cur, s_dbase, n, b, pb + s0, pb + s0, a.hash_base | ((unsigned long long)b << a.low_bits), true, nullptr);
}

// ---- buckets beyond the LDS sort ------------------------------------------------------------------------------------
// A hash shared by thousands of genomes -- a species of 1,000 strains and more -- is a posting list that alone overflows a
// bucket of 4,096 keys; until round 5 ONE such bucket sent the whole collection to the device-wide radix sort.  k_part_starts
// now lists the big buckets and this kernel builds them, one workgroup per bucket, streaming the bucket's keys from HBM as
// often as it has slabs:
//   * a histogram over the top 10 bits of hash_low places every sub-bucket (posting offsets are exact before anything is sorted);
//   * consecutive sub-buckets that fit the LDS together are a SLAB: gathered, sorted (bitonic, in LDS) and emitted like a bucket
//     of their own (emit_sorted_bucket);
//   * a sub-bucket that does not fit is split by its remaining hash bits; a single hash VALUE that does not fit is a heavy list:
//     its members are set in a bitmap over the genomes (LDS, one bit per genome: 64 KB for 524,288), which IS the sorted list --
//     the postings are its set bits, the runs its non-zero words, the tile records the pairs of non-zero words.
inline size_t heavy_lds_bytes(uint32_t n_blocks) { return (((size_t)std::max(n_blocks, kBucketCap) * 4 + (size_t)n_blocks * 2) + 15) & ~(size_t)15; }
struct HeavyArgs {
    TileEmitArgs e;
    const uint32_t *big_list;   // the pass's buckets of more than kBucketCap keys
    const uint32_t *n_big;
    uint32_t *next;             // the next bucket of the list to hand out (zeroed)
    uint32_t n_blocks;
};

// bitonic sort of S[0 .. n_pow2) by all T threads.  A wave owns a contiguous chunk of n_pow2 / (T / 64) elements: every stage
// whose partners lie inside a chunk (stride below half a chunk: 63 of the 78 stages at 4,096 keys) needs no workgroup barrier
// -- a wave's LDS operations execute in order.
template <int T> __device__ inline void bitonic_sort_lds(uint32_t *S, uint32_t n_pow2)
{
    constexpr uint32_t NW = T / 64;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto cmpx = [&](uint32_t t, uint32_t j, uint32_t k) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint32_t x = S[lo], y = S[hi];
        const bool up = (lo & k) == 0;
        if ((x > y) == up) { S[lo] = y; S[hi] = x; }
    };
    const bool one_wave = n_pow2 <= 128;                       // (a handful of keys: wave 0 alone)
    const uint32_t chunk = one_wave ? n_pow2 : n_pow2 / NW;    // elements a wave owns (>= 16)
    const uint32_t my_lo = one_wave ? 0u : wave * (chunk / 2), my_hi = one_wave ? (wave == 0 ? chunk / 2 : 0u) : my_lo + chunk / 2;   // its pairs
    for (uint32_t k = 2; k <= n_pow2; k <<= 1) {
        uint32_t j = k >> 1;
        for (; 2 * j > chunk; j >>= 1) {   // partners in different chunks: all threads, workgroup barriers
            for (uint32_t t = threadIdx.x; t < n_pow2 / 2; t += T) cmpx(t, j, k);
            __syncthreads();
        }
        for (; j > 0; j >>= 1) {           // inside the chunks
            for (uint32_t t = my_lo + lane; t < my_hi; t += 64) cmpx(t, j, k);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
    }
}

template <int T>
__global__ __launch_bounds__(T) void k_bucket_heavy(HeavyArgs h)
{
    using K = uint32_t;
    constexpr uint32_t NW = T / 64;
    constexpr uint32_t kSub = 1u << kSubBits;
    extern __shared__ __attribute__((aligned(16))) uint32_t heavy_lds[];   // bitmap u32[n_blocks], then nz u16[n_blocks]
    __shared__ __attribute__((aligned(16))) K S[kBucketCap];
    __shared__ uint16_t hd[kBucketCap + 2];
    __shared__ __attribute__((aligned(16))) uint32_t sb[2 * kSub + 2];   // (rpos of emit_sorted_bucket)
    __shared__ uint32_t sbc[kSub + 1], sbo[kSub + 1], hist2[64];
    __shared__ uint32_t wave_part[NW];
    __shared__ unsigned long long wave_part64[NW];
    __shared__ uint32_t s_cnt[kRecRegions], s_cur[kRecRegions];
    __shared__ unsigned long long s_dbase[kRecRegions];
    __shared__ uint32_t s_fill;
    const TileEmitArgs &a = h.e;
    uint32_t *bitmap = heavy_lds;   // (at least kBucketCap words: it also holds the run masks of a slab, heavy_lds_bytes)
    uint16_t *nz = reinterpret_cast<uint16_t *>(heavy_lds + max(h.n_blocks, kBucketCap));
    uint16_t *rpos = reinterpret_cast<uint16_t *>(sb);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.stop && a.stop->flags) {
        // (the build is refused, but k_heads_scan / k_heads_place still read every bucket's list count: the listed buckets get 0,
        // as k_bucket_emit_tiles gives the others -- a count left from earlier contents of the buffer would place heads anywhere)
        const uint32_t nb_listed = *h.n_big;
        for (uint32_t k = blockIdx.x * T + tid; k < nb_listed; k += gridDim.x * T) a.ucount[h.big_list[k]] = 0;
        return;
    }
    const uint32_t n_big = *h.n_big;
    if (n_big == 0) return;   // (the usual case at 10,000 genomes: not even a ticket's round trip)
    const uint32_t gmask = (1u << a.gb) - 1u;
    const int sub_bits = a.low_bits < kSubBits ? a.low_bits : kSubBits, rest_bits = a.low_bits - sub_bits;   // hash_low = sub-bucket | rest
    const uint32_t n_sub = 1u << sub_bits;
    const uint32_t pb = (uint32_t)a.pass_base[0];
    const uint32_t n_dest = a.n_dest, n_sub_regions = kRecRegions / n_dest;
    auto dest_of = [&](uint32_t row_block) { return n_dest > 1 ? row_block % n_dest : 0u; };
    if (tid < kRecRegions) s_cnt[tid] = s_cur[tid] = 0;
    // (the buckets are handed out one by one: their cost spans three orders of magnitude, and a fixed share per workgroup left most
    // of the chip waiting for the unluckiest one; every workgroup ends at the first ticket beyond the list)
    __shared__ uint32_t s_ticket;
    for (;;) {   // (uniform)
        __syncthreads();
        if (tid == 0) s_ticket = atomicAdd(h.next, 1u);
        __syncthreads();
        const uint32_t bi = s_ticket;
        if (bi >= n_big) break;
        const uint32_t b = h.big_list[bi];
        const uint32_t s0 = a.bstart[b], n = a.bstart[b + 1] - s0;
        const unsigned long long *keys = a.keys + s0;
        const unsigned long long hash_hi = a.hash_base | ((unsigned long long)b << a.low_bits);
        auto hl_of = [&](unsigned long long full) { return (uint32_t)(full >> (a.rb + a.gb)); };
        auto gi_of = [&](unsigned long long full) {
            const uint32_t gc = (uint32_t)(full >> a.rb) & gmask;
            return a.inv ? a.inv[gc] : gc;
        };
        for (uint32_t q = tid; q <= n_sub; q += T) sbc[q] = 0;
        __syncthreads();
        for (uint32_t k0 = 0; k0 < n; k0 += T) {   // (uniform trips)
            // these buckets are here BECAUSE one sub-bucket holds hundreds of their keys: the lanes that agree with the wave's first
            // key count with one LDS atomic instead of queueing 64 deep on one address
            const uint32_t k = k0 + tid;
            const bool have = k < n;
            const uint32_t v = have ? hl_of(keys[k]) >> rest_bits : 0xFFFFFFFFu;
            const uint32_t v0 = (uint32_t)__shfl((int)v, 0);
            const unsigned long long same = __ballot(have && v == v0);
            if (have && v == v0) {
                if (lane == (uint32_t)__ffsll((long long)same) - 1u) atomicAdd(&sbc[v], (uint32_t)__popcll(same));
            } else if (have) {
                atomicAdd(&sbc[v], 1u);
            }
        }
        __syncthreads();
        {   // exclusive scan of the sub-bucket counts (at most 1,024 = one per thread)
            static_assert(kSub <= T, "one sub-bucket per thread");
            const uint32_t c = tid < n_sub ? sbc[tid] : 0u;
            uint32_t incl = c;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o);
                if ((int)lane >= o) incl += t;
            }
            if (lane == 63) wave_part[wave] = incl;
            __syncthreads();
            uint32_t before = incl - c;
            for (uint32_t w = 0; w < wave; w++) before += wave_part[w];
            if (tid < n_sub) sbo[tid] = before;
            if (tid == n_sub - 1) sbo[n_sub] = before + c;
            __syncthreads();
        }
        uint32_t heads_done = 0;

        // a slab: the keys with hash_low in [hl_lo, hl_hi), `tot` <= kBucketCap of them, postings from post_off on
        auto light_slab = [&](uint32_t hl_lo, uint32_t hl_hi, uint32_t tot, uint32_t post_off) {
            if (tid == 0) s_fill = 0;
            uint32_t p2 = 1;
            while (p2 < tot) p2 <<= 1;
            for (uint32_t q = tot + tid; q < p2; q += T) S[q] = 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k0 = 0; k0 < n; k0 += T) {   // (uniform trips; one LDS atomic per wave: a slab is mostly ONE list, every key wants in)
                const uint32_t k = k0 + tid;
                const unsigned long long full = k < n ? keys[k] : 0ULL;
                const uint32_t hl = hl_of(full);
                const bool take = k < n && hl >= hl_lo && hl < hl_hi;
                const unsigned long long m = __ballot(take);
                if (!m) continue;
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(&s_fill, (uint32_t)__popcll(m));
                at = (uint32_t)__shfl((int)at, 0);
                if (take) S[at + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL))] = (hl << a.gb) | gi_of(full);
            }
            __syncthreads();
            if (!(a.debug & 64)) bitonic_sort_lds<T>(S, p2);   // (RK_INDEX_DEBUG 64: developer ablation, the slab unsorted)
            const uint32_t U = emit_sorted_bucket<T, K>(a, S, hd, rpos, wave_part, s_cnt, s_cur, s_dbase, tot, b, pb + s0 + post_off, pb + s0 + heads_done,
                                                        hash_hi, false, bitmap);   // (the bitmap's LDS holds the run masks: a slab has at most 4,096 runs)
            __syncthreads();
            heads_done += U;
        };
        // one hash value with more members than the LDS sort holds: the genome bitmap
        auto heavy_list = [&](uint32_t hl, uint32_t post_off) {
            for (uint32_t w = tid; w < h.n_blocks; w += T) bitmap[w] = 0;
            __syncthreads();
            for (uint32_t k = tid; k < n; k += T) {
                const unsigned long long full = keys[k];
                if (hl_of(full) == hl) {
                    const uint32_t g = gi_of(full);
                    atomicOr(&bitmap[g >> 5], 1u << (g & 31u));
                }
            }
            __syncthreads();
            // members and non-zero words before every thread's stretch of words
            const uint32_t wpt = (h.n_blocks + T - 1) / T, w0 = min(h.n_blocks, tid * wpt), w1 = min(h.n_blocks, w0 + wpt);
            unsigned long long mine = 0;
            for (uint32_t w = w0; w < w1; w++) {
                const uint32_t m = bitmap[w];
                mine += (unsigned long long)__popc(m) + (m ? (1ULL << 32) : 0ULL);
            }
            unsigned long long incl = mine;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long t = (unsigned long long)__shfl_up((long long)incl, o);
                if ((int)lane >= o) incl += t;
            }
            if (lane == 63) wave_part64[wave] = incl;
            __syncthreads();
            unsigned long long before = incl - mine, all = 0;
            for (uint32_t w = 0; w < NW; w++) {
                if (w < wave) before += wave_part64[w];
                all += wave_part64[w];
            }
            const uint32_t R = (uint32_t)(all >> 32);
            {
                uint32_t at_p = (uint32_t)before, at_r = (uint32_t)(before >> 32);
                for (uint32_t w = w0; w < w1; w++) {
                    uint32_t m = bitmap[w];
                    if (m) nz[at_r++] = (uint16_t)w;
                    while (m) {
                        const int bit = __builtin_ctz(m);
                        m &= m - 1;
                        a.postings[pb + s0 + post_off + at_p++] = (w << 5) + (uint32_t)bit;
                    }
                }
            }
            if (tid == 0) {
                const unsigned long long hh = hash_hi | hl;
                if (a.tmp_uhash64) a.tmp_uhash64[pb + s0 + heads_done] = hh;
                else a.tmp_uhash[pb + s0 + heads_done] = (uint32_t)hh;
                a.tmp_upos[pb + s0 + heads_done] = pb + s0 + post_off;
            }
            __syncthreads();
            // tile records: row run i pairs with every later run j, and with itself when it holds two members
            for (uint32_t i = tid; i < R; i += T) {
                const uint32_t w = nz[i];
                atomicAdd(&s_cnt[dest_of(w)], (R - 1 - i) + (__popc(bitmap[w]) >= 2 ? 1u : 0u));
            }
            __syncthreads();
            if (tid < n_dest) {
                const uint32_t want = s_cnt[tid];
                s_cnt[tid] = 0;
                s_cur[tid] = 0;
                const uint32_t region = tid * n_sub_regions + b % n_sub_regions;
                unsigned long long base = ~0ULL;
                if (want) {
                    const unsigned long long got = atomicAdd(&a.tres->rec_count[region], (unsigned long long)want);
                    if (got + want <= a.region_cap) base = (unsigned long long)region * a.region_cap + got;
                    else a.tres->overflow = 1;
                }
                s_dbase[tid] = base;
            }
            __syncthreads();
            for (uint32_t i = wave; i < R && !(a.debug & 1); i += NW) {   // a wave per row run
                const uint32_t wi = nz[i], mi = bitmap[wi], d = dest_of(wi);
                const bool self = __popc(mi) >= 2;
                const uint32_t cnt = (R - 1 - i) + (self ? 1u : 0u);
                uint32_t at = 0;
                if (lane == 0 && cnt) at = atomicAdd(&s_cur[d], cnt);
                at = (uint32_t)__shfl((int)at, 0);
                const unsigned long long base = s_dbase[d];
                if (base == ~0ULL) continue;
                for (uint32_t j = i + 1 + lane; j < R; j += 64) {
                    const uint32_t wj = nz[j];
                    a.rec[base + at + (j - i - 1)] = make_uint3((wi << 16) | wj, mi, bitmap[wj]);
                }
                if (self && lane == 0) a.rec[base + at + (R - 1 - i)] = make_uint3((wi << 16) | wi, mi, mi);
            }
            __syncthreads();
            heads_done += 1;
        };

        uint32_t sidx = 0;
        while (sidx < n_sub) {   // (uniform: every thread reads the same LDS words)
            // the slab from sidx on: the furthest sub-bucket end within kBucketCap keys (the offsets ascend: a binary search)
            const uint32_t base = sbo[sidx];
            uint32_t lo = sidx, hi = n_sub;   // sbo[lo] - base <= cap always; the answer: largest e with sbo[e] - base <= cap
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (sbo[mid] - base <= kBucketCap) lo = mid; else hi = mid - 1;
            }
            if (lo > sidx) {
                const uint32_t tot = sbo[lo] - base;
                if (tot) light_slab(sidx << rest_bits, lo << rest_bits, tot, base);
                sidx = lo;
                continue;
            }
            if (rest_bits == 0) {
                heavy_list(sidx, sbo[sidx]);
            } else if (rest_bits > 6) {   // (more than 64 values per sub-bucket: not handled here -- the general path decides)
                if (tid == 0) atomicOr((unsigned long long *)&a.stop_rw->flags, (unsigned long long)kFastOverflow);
            } else {
                const uint32_t n_val = 1u << rest_bits;
                if (tid < 64) hist2[tid] = 0;
                __syncthreads();
                for (uint32_t k = tid; k < n; k += T) {
                    const uint32_t hl = hl_of(keys[k]);
                    if ((hl >> rest_bits) == sidx) atomicAdd(&hist2[hl & (n_val - 1u)], 1u);
                }
                __syncthreads();
                uint32_t off2 = sbo[sidx], v = 0;
                while (v < n_val) {
                    const uint32_t c2 = hist2[v];
                    if (!c2) { v++; continue; }
                    if (c2 <= kBucketCap) {
                        uint32_t e2 = v, tot = 0;
                        while (e2 < n_val && tot + hist2[e2] <= kBucketCap) tot += hist2[e2++];
                        light_slab((sidx << rest_bits) + v, (sidx << rest_bits) + e2, tot, off2);
                        off2 += tot;
                        v = e2;
                    } else {
                        heavy_list((sidx << rest_bits) + v, off2);
                        off2 += c2;
                        v++;
                    }
                }
            }
            sidx++;
        }
        if (tid == 0) a.ucount[b] = heads_done;
        __syncthreads();
    }
}

struct TileSortArgs {
    const uint3 *rec;       // the unsorted records, kRecRegions regions (counts: tres->rec_count)
    TileCursors *cur;
    uint32_t region_cap;
    uint32_t n_blocks;
    uint32_t *bin_count;    // [n_blocks + 1], zeroed
    uint32_t *bin_start;    // [n_blocks + 1]
    uint32_t *bin_cursor;   // [n_blocks], zeroed
    uint3 *brec;            // the records binned by row block
    const uint32_t *blk_min;   // smallest non-empty sketch of every block (0xFFFFFFFF: none)
    uint2 *contrib;         // final: (row mask, column mask), every tile from an even slot
    uint32_t *rows, *cols;  // final, split copy in the same slots (null beyond 8,192 blocks: only the scalar-row variant of the tile kernel reads it, and that is for short launches over small collections)
    uint32_t *tb_base, *tb_cnt;   // proto entries of the i-th row block of `order`: [tb_base[i], + tb_cnt[i])
    uint32_t *order;        // [n_blocks] the row blocks in the order k_trec_rowsort draws them: the fullest bins first (k_trec_starts)
    uint4 *proto;           // two uint4 per tile: {b, w, first slot (2 words)} {records, bound jaccard, bound containment, level j | level c << 16}
    unsigned long long *level_start;   // [2][kTileTable + 1]
    uint4 *dir[2];
    TileResult *tres;
    uint32_t stage_slots;   // slots of the row sort's LDS stage (rowsort_stage)
    int debug;              // developer ablations (RK_ROWSORT_DEBUG; the records are then wrong by design): 1 no placement, 2 no split copy, 4 no histogram atomics
};

// this workgroup's share of region blockIdx.x: records [lo, hi) of the region
__device__ inline void trec_share(const TileSortArgs &a, unsigned long long *lo, unsigned long long *hi)
{
    const unsigned long long cnt = min(a.tres->rec_count[blockIdx.x], (unsigned long long)a.region_cap);
    const unsigned long long share = (cnt + gridDim.y - 1) / gridDim.y;
    const unsigned long long base = (unsigned long long)blockIdx.x * a.region_cap;
    *lo = base + min(cnt, (unsigned long long)blockIdx.y * share);
    *hi = base + min(cnt, ((unsigned long long)blockIdx.y + 1) * share);
}

// LDS histogram of the row blocks of records [lo, hi) (eight loads in flight per thread)
__device__ inline void trec_histogram(const TileSortArgs &a, unsigned long long lo, unsigned long long hi, uint32_t *h)
{
    constexpr int D = 8;
    for (unsigned long long i0 = lo + threadIdx.x; i0 < hi; i0 += (unsigned long long)D * blockDim.x) {
        uint32_t k[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            const unsigned long long i = i0 + (unsigned long long)d * blockDim.x;
            k[d] = i < hi ? a.rec[i].x : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int d = 0; d < D; d++)
            if (k[d] != 0xFFFFFFFFu) atomicAdd(&h[k[d] >> 16], 1u);
    }
}

__global__ __launch_bounds__(512) void k_trec_count(TileSortArgs a)
{
    extern __shared__ uint32_t trec_lds[];
    if (a.tres->overflow) return;
    for (uint32_t i = threadIdx.x; i < a.n_blocks; i += blockDim.x) trec_lds[i] = 0;
    __syncthreads();
    unsigned long long lo, hi;
    trec_share(a, &lo, &hi);
    trec_histogram(a, lo, hi, trec_lds);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_blocks; i += blockDim.x)
        if (trec_lds[i]) atomicAdd(&a.bin_count[i], trec_lds[i]);
}

__global__ void k_trec_starts(TileSortArgs a)
{
    if (a.tres->overflow) return;
    const uint32_t all = block_scan_sweeps<uint32_t>(a.n_blocks, [&](uint32_t i) { return a.bin_count[i]; },
                                                     [&](uint32_t i, uint32_t before) { a.bin_start[i] = before; });
    if (threadIdx.x == 0) {
        a.bin_start[a.n_blocks] = all;
        a.tres->n_records = all;
    }
    // the order of the row sort: bins far above the mean first (the species of thousands of strains: a workgroup that starts on
    // 400,000 records when the rest of the grid has drained IS the kernel's duration), the rest as they come
    __shared__ uint32_t n_first, n_rest;
    if (threadIdx.x == 0) n_first = n_rest = 0;
    __syncthreads();
    const uint32_t big = max(16384u, 8u * (all / a.n_blocks));
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; round < 2; round++) {
        for (uint32_t i0 = threadIdx.x - lane; i0 < a.n_blocks; i0 += blockDim.x) {   // (wave-uniform trips)
            const uint32_t i = i0 + lane;
            const bool mine = i < a.n_blocks && (a.bin_count[i] > big) == (round == 0);
            const unsigned long long m = __ballot(mine);
            if (!m) continue;
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(round ? &n_rest : &n_first, (uint32_t)__popcll(m));
            at = (uint32_t)__shfl((int)at, 0) + (round ? n_first : 0u);
            if (mine) a.order[at + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL))] = i;
        }
        __syncthreads();
    }
}

// (a record moves with ONE 12-byte store: scattered stores cost by their number -- 13 us per million on this chip, whatever
// their size; with key and masks in separate arrays this pass took 52 us for 1.8 M records)
__global__ __launch_bounds__(512) void k_trec_scatter(TileSortArgs a)
{
    extern __shared__ uint32_t trec_lds[];
    if (a.tres->overflow) return;
    for (uint32_t i = threadIdx.x; i < a.n_blocks; i += blockDim.x) trec_lds[i] = 0;
    __syncthreads();
    unsigned long long lo, hi;
    trec_share(a, &lo, &hi);
    trec_histogram(a, lo, hi, trec_lds);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_blocks; i += blockDim.x) {   // one run per bin: where it goes
        const uint32_t c = trec_lds[i];
        if (c) trec_lds[i] = a.bin_start[i] + atomicAdd(&a.bin_cursor[i], c);
    }
    __syncthreads();
    constexpr int D = 8;   // (loads in flight per thread: a thread's share is a handful of records, one round trip instead of one per record)
    for (unsigned long long i0 = lo + threadIdx.x; i0 < hi; i0 += (unsigned long long)D * blockDim.x) {
        uint3 r[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            const unsigned long long i = i0 + (unsigned long long)d * blockDim.x;
            r[d] = i < hi ? a.rec[i] : make_uint3(0xFFFFFFFFu, 0, 0);
        }
#pragma unroll
        for (int d = 0; d < D; d++)
            if (r[d].x != 0xFFFFFFFFu) a.brec[atomicAdd(&trec_lds[r[d].x >> 16], 1u)] = r[d];
    }
}

// The row blocks' records by column block.  A workgroup draws row blocks from the list of k_trec_starts (the fullest first) until it
// is empty; a bin of up to kRowStage slots is sorted in LDS and leaves in three coalesced streams (AoS + the split copy), a bigger
// one is placed directly -- ONE scattered store per record (they cost by their number: 13 us per million) -- and its split copy read
// back in order from what the workgroup just wrote.  ONE LDS word per column block: the count, then the tile's cursor (the proto
// directory entries are written between the two) -- 62 KB at 500,000 genomes, two workgroups of 1,024 threads per CU.
constexpr uint32_t kRowStage = 6144;
inline uint32_t rowsort_stage(uint32_t n_blocks) { return n_blocks <= 8192 ? kRowStage : 0; }
inline size_t rowsort_lds(uint32_t n_blocks) { return (size_t)n_blocks * 4 + 8 + (size_t)rowsort_stage(n_blocks) * 8; }
template <uint32_t T> __global__ __launch_bounds__(T) void k_trec_rowsort(TileSortArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t trec_lds[];
    __shared__ unsigned long long scan_part[T / 64];
    __shared__ unsigned long long s_slot0, s_tile0;
    __shared__ uint32_t lv[2][kTileTable + 1];
    __shared__ uint32_t s_ticket;
    if (a.tres->overflow) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = a.n_blocks;
    uint32_t *cur = trec_lds;
    uint2 *stage = reinterpret_cast<uint2 *>(trec_lds + ((nb + 1) & ~1u));
    // (eight or sixteen loads in flight per thread: a workgroup that reads a bin of 400,000 records is bound by what ONE CU keeps in flight)
    constexpr int D = T >= 1024 ? 16 : 8;
    for (;;) {   // (uniform; every workgroup ends at the first ticket beyond the list)
        __syncthreads();   // (the LDS of the row block before)
        if (tid == 0) s_ticket = (uint32_t)atomicAdd(&a.cur->ticket, 1ULL);
        __syncthreads();
        const uint32_t it = s_ticket;
        if (it >= nb) break;
        const uint32_t b = a.order[it];
        const uint32_t r0 = a.bin_start[b], r1 = a.bin_start[b + 1];
        if (r0 == r1) {   // (uniform)
            if (tid == 0) a.tb_cnt[it] = 0;
            continue;
        }
        for (uint32_t i = tid; i < nb; i += T) cur[i] = 0;
        for (uint32_t i = tid; i < 2 * (kTileTable + 1); i += T) (&lv[0][0])[i] = 0;
        __syncthreads();
        for (uint32_t i0 = r0 + tid; i0 < r1; i0 += D * T) {
            uint32_t k[D];
#pragma unroll
            for (int d = 0; d < D; d++) k[d] = i0 + d * T < r1 ? a.brec[i0 + d * T].x : 0xFFFFFFFFu;
#pragma unroll
            for (int d = 0; d < D; d++)
                if (k[d] != 0xFFFFFFFFu && !(a.debug & 4)) atomicAdd(&cur[k[d] & 0xFFFFu], 1u);
        }
        __syncthreads();
        // exclusive scan over the column blocks: slots (every tile padded to an even count) in the low 40 bits, tiles above
        const uint32_t per = ((nb + T - 1) / T) | 1u;   // (odd: the threads' stretches start in 32 different LDS banks)
        const uint32_t w0 = min(nb, tid * per), w1 = min(nb, w0 + per);
        unsigned long long mine = 0;
        uint32_t biggest = 0;
        for (uint32_t w = w0; w < w1; w++) {
            const uint32_t c = cur[w];
            mine += (unsigned long long)((c + 1u) & ~1u) + (c ? (1ULL << 40) : 0ULL);
            biggest = max(biggest, c);
        }
        unsigned long long incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = (unsigned long long)__shfl_up((long long)incl, o);
            if ((int)lane >= o) incl += t;
        }
        for (int o = 32; o > 0; o >>= 1) biggest = max(biggest, (uint32_t)__shfl_xor((int)biggest, o));
        if (lane == 63) scan_part[wave] = incl;
        __syncthreads();
        unsigned long long before = incl - mine, all = 0;
        for (uint32_t w = 0; w < T / 64; w++) {
            if (w < wave) before += scan_part[w];
            all += scan_part[w];
        }
        const unsigned long long n_slots = all & ((1ULL << 40) - 1ULL), n_tiles = all >> 40;
        const bool staged = n_slots <= a.stage_slots;   // (uniform)
        if (tid == 0) {
            s_slot0 = atomicAdd(&a.cur->final_at, n_slots);
            s_tile0 = atomicAdd(&a.cur->tile_at, n_tiles);
            a.tb_base[it] = (uint32_t)s_tile0;
            a.tb_cnt[it] = (uint32_t)n_tiles;
        }
        if (lane == 0 && biggest) atomicMax(&a.tres->max_records, (unsigned long long)biggest);
        if (staged)
            for (uint32_t i = tid; i < (uint32_t)n_slots; i += T) stage[i] = make_uint2(0, 0);   // (the slot that pads an odd tile)
        __syncthreads();
        const unsigned long long slot0 = s_slot0, tile0 = s_tile0;
        // the stretches again: the proto directory entries, and every count becomes its tile's cursor
        {
            uint32_t at = (uint32_t)(before & ((1ULL << 40) - 1ULL));   // (a row block's records fit 32 bits: the unsorted capacity does)
            unsigned long long t = tile0 + (before >> 40);
            const uint32_t mb = a.blk_min[b];
            for (uint32_t w = w0; w < w1; w++) {
                const uint32_t c = cur[w];
                cur[w] = at;
                if (c) {
                    const unsigned long long first = slot0 + at;
                    const uint32_t mw = a.blk_min[w];
                    const uint32_t lb_j = max(mb, mw), lb_c = min(mb, mw);
                    const uint32_t lj = tile_level(c, lb_j), lc = tile_level(c, lb_c);
                    a.proto[2 * t] = make_uint4(b, w, (uint32_t)first, (uint32_t)(first >> 32));
                    a.proto[2 * t + 1] = make_uint4(c, lb_j, lb_c, lj | (lc << 16));
                    atomicAdd(&lv[0][lj], 1u);
                    atomicAdd(&lv[1][lc], 1u);
                    t++;
                }
                at += (c + 1u) & ~1u;
            }
        }
        __syncthreads();
        if (staged) {
            for (uint32_t i0 = r0 + tid; i0 < r1; i0 += D * T) {
                uint3 r[D];
#pragma unroll
                for (int d = 0; d < D; d++) r[d] = i0 + d * T < r1 ? a.brec[i0 + d * T] : make_uint3(0xFFFFFFFFu, 0, 0);
#pragma unroll
                for (int d = 0; d < D; d++)
                    if (r[d].x != 0xFFFFFFFFu) stage[atomicAdd(&cur[r[d].x & 0xFFFFu], 1u)] = make_uint2(r[d].y, r[d].z);
            }
            __syncthreads();
            for (uint32_t i = tid; i < (uint32_t)n_slots; i += T) {
                const uint2 v = stage[i];
                a.contrib[slot0 + i] = v;
                a.rows[slot0 + i] = v.x;
                a.cols[slot0 + i] = v.y;
            }
        } else {
            for (uint32_t i0 = r0 + tid; i0 < r1; i0 += D * T) {
                uint3 r[D];
#pragma unroll
                for (int d = 0; d < D; d++) r[d] = i0 + d * T < r1 ? a.brec[i0 + d * T] : make_uint3(0xFFFFFFFFu, 0, 0);
#pragma unroll
                for (int d = 0; d < D; d++)
                    if (r[d].x != 0xFFFFFFFFu && !(a.debug & 1)) a.contrib[slot0 + atomicAdd(&cur[r[d].x & 0xFFFFu], 1u)] = make_uint2(r[d].y, r[d].z);
            }
            __syncthreads();
            for (unsigned long long i0 = tid; i0 < n_slots && a.rows && !(a.debug & 2); i0 += (unsigned long long)D * T) {   // (a.rows: collections beyond 8,192 blocks carry no split copy)
                uint2 v[D];
#pragma unroll
                for (int d = 0; d < D; d++) v[d] = i0 + (unsigned long long)d * T < n_slots ? a.contrib[slot0 + i0 + (unsigned long long)d * T] : make_uint2(0, 0);
#pragma unroll
                for (int d = 0; d < D; d++)
                    if (i0 + (unsigned long long)d * T < n_slots) {
                        a.rows[slot0 + i0 + (unsigned long long)d * T] = v[d].x;
                        a.cols[slot0 + i0 + (unsigned long long)d * T] = v[d].y;
                    }
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < 2 * (kTileTable + 1); i += T) {
            const uint32_t c = (&lv[0][0])[i];
            if (c) atomicAdd(&a.tres->level_count[0][0] + i, (unsigned long long)c);
        }
    }
}

// one workgroup: level starts; level_count becomes "tiles of this level or denser" (the host's launch sizes)
__global__ void k_tdir_scan(TileSortArgs a)
{
    if (a.tres->overflow) return;
    const uint32_t m = threadIdx.x >> 9, l = threadIdx.x & 511;   // 1,024 threads: metric, level
    __shared__ unsigned long long part[2][512 / 64];
    const unsigned long long c = l <= (uint32_t)kTileTable ? a.tres->level_count[m][l] : 0ULL;
    unsigned long long incl = c;
    const uint32_t lane = threadIdx.x & 63, wv = l >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = (unsigned long long)__shfl_up((long long)incl, o);
        if ((int)lane >= o) incl += t;
    }
    if (lane == 63) part[m][wv] = incl;
    __syncthreads();
    for (uint32_t w = 0; w < wv; w++) incl += part[m][w];
    if (l <= (uint32_t)kTileTable) {
        a.level_start[m * (kTileTable + 1) + l] = incl - c;
        a.tres->level_count[m][l] = incl;
    }
    if (threadIdx.x == 0) {
        a.tres->n_tiles = a.cur->tile_at;
        a.tres->n_slots = a.cur->final_at;
    }
}

// a workgroup per kDirItems row blocks (in the row sort's order): their tiles to their places in the two launch orders (one reservation per
// level and workgroup: the counters of the few dense levels are same-address atomics -- 13 ns each, and with a workgroup per row
// block 15,625 of them queued on each: 0.47 ms at 500,000 genomes)
constexpr uint32_t kDirItems = 8;
__global__ __launch_bounds__(256) void k_tdir_place(TileSortArgs a)
{
    constexpr uint32_t T = 256;
    __shared__ unsigned long long at[2][kTileTable + 1];
    __shared__ uint32_t cnt[2][kTileTable + 1];
    if (a.tres->overflow) return;
    const uint32_t n_items = a.n_blocks, tid = threadIdx.x;
    const uint32_t it0 = blockIdx.x * kDirItems, it1 = min(n_items, it0 + kDirItems);
    if (it0 >= it1) return;
    for (uint32_t i = tid; i < 2 * (kTileTable + 1); i += T) (&cnt[0][0])[i] = 0;
    __syncthreads();
    for (uint32_t it = it0; it < it1; it++) {
        const uint32_t n = a.tb_cnt[it];
        const uint4 *mine = a.proto + 2 * (size_t)a.tb_base[it];
        for (uint32_t t = tid; t < n; t += T) {
            const uint32_t lv = mine[2 * t + 1].w;
            atomicAdd(&cnt[0][lv & 0xFFFFu], 1u);
            atomicAdd(&cnt[1][lv >> 16], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 2 * (kTileTable + 1); i += T) {
        const uint32_t c = (&cnt[0][0])[i];
        if (c) (&at[0][0])[i] = a.level_start[i] + atomicAdd(&a.cur->level_at[0][0] + i, (unsigned long long)c);
    }
    __syncthreads();
    for (uint32_t it = it0; it < it1; it++) {
        const uint32_t n = a.tb_cnt[it];
        const uint4 *mine = a.proto + 2 * (size_t)a.tb_base[it];
        for (uint32_t t = tid; t < n; t += T) {
            const uint4 e0 = mine[2 * t], e1 = mine[2 * t + 1];
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const uint32_t lv = m ? (e1.w >> 16) : (e1.w & 0xFFFFu);
                const unsigned long long p = atomicAdd(&at[m][lv], 1ULL);
                a.dir[m][2 * p] = e0;
                a.dir[m][2 * p + 1] = make_uint4(e1.x, m ? e1.z : e1.y, e0.z, e0.w);   // (records, denominator bound, first slot of the split copy)
            }
        }
    }
}

__global__ void k_blk_min_sizes(const uint32_t *sizes, uint32_t n_ref, uint32_t n_blocks, uint32_t *blk_min)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    uint32_t m = 0xFFFFFFFFu;
    for (uint32_t g = b * 32; g < min(n_ref, b * 32 + 32); g++) {
        const uint32_t s = sizes[g];
        if (s && s < m) m = s;
    }
    blk_min[b] = m;
}

// the tile sort on `st`: records of ta.rec (kRecRegions regions, counts in ta.tres->rec_count) -> contrib / rows / cols / dir.
// before_rowsort(): the caller's join with whatever produces ta.blk_min.
template <class F> int launch_tile_sort(rk_ctx *ctx, TileSortArgs ta, hipStream_t st, F before_rowsort)
{
    const size_t hist_lds = (size_t)ta.n_blocks * 4;
    ta.stage_slots = rowsort_stage(ta.n_blocks);
    ta.debug = getenv("RK_ROWSORT_DEBUG") ? atoi(getenv("RK_ROWSORT_DEBUG")) : 0;
    if (hist_lds > 48 * 1024) {
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_trec_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds));
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_trec_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds));
    }
    hipLaunchKernelGGL(k_trec_count, dim3(kRecRegions, kRecParts), dim3(512), hist_lds, st, ta);
    hipLaunchKernelGGL(k_trec_starts, dim3(1), dim3(1024), 0, st, ta);
    hipLaunchKernelGGL(k_trec_scatter, dim3(kRecRegions, kRecParts), dim3(512), hist_lds, st, ta);
    int rc = before_rowsort();   // (the blocks' smallest sketches come from the second stream; by now also the list heads)
    if (rc) return rc;
    // (beyond 8,192 blocks the two histograms leave room for ONE workgroup per CU: it then has 16 waves, not 8)
    if (ta.stage_slots) {
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_trec_rowsort<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowsort_lds(ta.n_blocks)));
        hipLaunchKernelGGL(k_trec_rowsort<512>, dim3(std::min(ta.n_blocks, 4096u)), dim3(512), rowsort_lds(ta.n_blocks), st, ta);
    } else {
        RK_HIP(ctx, hipFuncSetAttribute((const void *)k_trec_rowsort<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowsort_lds(ta.n_blocks)));
        hipLaunchKernelGGL(k_trec_rowsort<1024>, dim3(std::min(ta.n_blocks, 1024u)), dim3(1024), rowsort_lds(ta.n_blocks), st, ta);
    }
    hipLaunchKernelGGL(k_tdir_scan, dim3(1), dim3(1024), 0, st, ta);
    hipLaunchKernelGGL(k_tdir_place, dim3((ta.n_blocks + kDirItems - 1) / kDirItems), dim3(256), 0, st, ta);
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}
