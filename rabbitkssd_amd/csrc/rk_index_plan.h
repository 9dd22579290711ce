// rk_index_plan.h -- which index build a collection gets: the developer knobs, the plan of a build and of one bucket-sort
// attempt, the layout of the buffer the kernels expect zeroed, typed dispatch.  Host arithmetic only: nothing here launches or
// allocates.  Included by rk_index.hip alone, inside its anonymous namespace, behind the .inc files whose constants and
// result records it uses.

inline int genome_bits_of(uint64_t n)   // the smallest b >= 1 with 2^b >= n: genome ids, positions inside a sketch
{
    int b = 1;
    while ((1ULL << b) < n) b++;
    return b;
}
inline int shard_bits_of(uint32_t n_shards)
{
    int b = 0;
    while ((1u << b) < n_shards) b++;
    return b;
}

// typed dispatch (with_hash_type: rk_internal.h): f(K()) with the key type of the bucket sort (32 bits when (hash_low, genome)
// fit them -- also what k_heads_place is instantiated with), f(T, K()) with the emission's block size as well
template <class F> int with_key_type(bool narrow, F f) { return narrow ? f(uint32_t()) : f((unsigned long long)0); }
template <int T> using Threads = std::integral_constant<int, T>;
template <class F> int with_emit_shape(int emit_t, bool narrow, F f)
{
    return with_key_type(narrow, [&](auto key) -> int {
        return emit_t == 256 ? f(Threads<256>(), key) : emit_t == 1024 ? f(Threads<1024>(), key) : f(Threads<512>(), key);
    });
}

// developer knobs of the build: read from the environment at the top of EVERY build (tests change them between builds on one context)
struct BuildKnobs {
    int pass_bits;             // RK_INDEX_PASS_BITS, 0 .. 7 (tests: several passes over a small collection); -1: as many as it takes
    uint64_t bucket_target;    // RK_INDEX_BUCKET_TARGET, at least 64
    bool one_stream;           // RK_INDEX_ONE_STREAM: the renumbering stays on the context's stream
    bool stream2_high;         // RK_INDEX_STREAM2_PRIO=0: the second stream at the default priority
    unsigned long long table_x;   // RK_INDEX_TABLE_X: slots of the renumbering's table per (genome, smallest hash)
    int xcd_map;               // RK_INDEX_XCD: xcd_item()
    uint64_t keys_cap_pct;     // RK_INDEX_KEYS_CAP_PCT (tests make the estimate of a range pass too small)
    bool part2, filter;        // RK_INDEX_PART2=0, RK_INDEX_FILTER=0: the one-pass partition, range passes that walk every hash
    int emit_t;                // RK_INDEX_EMIT_T: 256, 1024 or (anything else) 512 threads per bucket
    int debug;                 // RK_INDEX_DEBUG: the emission's ablations
};
BuildKnobs read_knobs()
{
    auto num = [](const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; };
    BuildKnobs k;
    k.pass_bits = getenv("RK_INDEX_PASS_BITS") ? std::max(0, std::min(7, num("RK_INDEX_PASS_BITS", 0))) : -1;
    k.bucket_target = std::max(64, num("RK_INDEX_BUCKET_TARGET", kBucketTarget));
    k.one_stream = getenv("RK_INDEX_ONE_STREAM") != nullptr;
    k.stream2_high = num("RK_INDEX_STREAM2_PRIO", 1) != 0;
    k.table_x = getenv("RK_INDEX_TABLE_X") ? strtoull(getenv("RK_INDEX_TABLE_X"), nullptr, 10) : 2ULL;
    k.xcd_map = num("RK_INDEX_XCD", 1);
    k.keys_cap_pct = std::max(1, num("RK_INDEX_KEYS_CAP_PCT", 125));
    k.part2 = num("RK_INDEX_PART2", 1) != 0;
    k.filter = num("RK_INDEX_FILTER", 1) != 0;
    k.emit_t = num("RK_INDEX_EMIT_T", 512);
    k.debug = num("RK_INDEX_DEBUG", 0);
    return k;
}

// Which build a collection gets: everything that is fixed before the first launch.
struct BuildPlan {
    bool from_keys, wide;      // from_keys: a shard of a sharded build from exchanged keys -- never the general path
    uint32_t N, n_blocks, shard_id, n_shards, n_pass;
    uint64_t H;                // postings of the whole collection
    uint64_t H_el;             // the elements the partition reads: the whole collection, or the shard's keys (arrays that scale with postings are sized by these)
    uint64_t Ucap;             // distinct hashes: at most H_el, at most the hash space
    uint64_t H_pass;           // keys of one pass (estimate: the hashes are spread evenly)
    uint64_t H_el_shard;       // postings of this shard: known from keys, else estimated
    int hash_bits, shard_bits, pass_bits, range_bits;
    int eff_bits;              // hash bits inside a range
    int B, gb, rb, low_bits;   // bucket, genome, position bits; hash bits below the bucket
    bool no_self;              // no slice records, ever (2^31-1 postings or more, RK_INDEX_NO_SELF)
    bool slices_ok, tiles_ok;  // the products the bucket sort can have
    bool tiles_mode;           // ... and the one its first attempt has
    bool relabel, two_streams; // the renumbering runs, and on a stream of its own
    bool fast_ok() const { return tiles_mode || slices_ok; }
};

// The plan of a build and the refusals that follow from it alone: launches nothing, allocates nothing.
int plan_build(rk_ctx *ctx, const BuildSource &src, int hash_bits, uint32_t shard_id, uint32_t n_shards, const BuildKnobs &k, BuildPlan *out)
{
    BuildPlan p;
    if (hash_bits < 1) return rk_fail(ctx, RK_ERR_ARG, "hash_bits must be positive");
    if (hash_bits > 64) return rk_fail(ctx, RK_ERR_ARG, "hash_bits=%d", hash_bits);
    if ((hash_bits > 32) != src.wide)
        return rk_fail(ctx, RK_ERR_ARG, "hash_bits=%d does not match the sketches' %s-bit layout", hash_bits,
                       src.wide ? "64" : "32");
    p.from_keys = src.s == nullptr;
    p.wide = src.wide;
    p.hash_bits = hash_bits;
    p.shard_id = shard_id;
    p.n_shards = n_shards;
    const uint64_t H = p.H = src.total;
    const uint32_t N = p.N = src.n;
    p.H_el = p.from_keys ? src.n_keys : H;
    // Bit 31 of a slice record tags its compact form, so posting offsets inside slice records stay below 2^31.  An index of
    // 2^31-1 .. 2^32-2 postings (all of GenBank's bacteria at ~1,200 hashes each) is built WITHOUT slice records: its
    // postings, list offsets and distinct hashes are complete (.dict / .index export, sparse self joins through the tile
    // kernel, which reads the posting lists themselves); what needs slice records -- a dense report, sketches that repeat
    // a hash -- is refused for it.  RK_INDEX_NO_SELF=1 builds any index that way (tests).
    if (H >= 0xFFFFFFFFULL || N >= 0x7FFFFFFFu) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "more than 2^32-2 postings or 2^31-1 genomes");
    p.no_self = H >= 0x7FFFFFFFULL || ctx->sw_index_no_self;
    if (p.no_self && !src.is_set)
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "an index of more than 2^31-1 postings needs set sketches (no hash twice in a genome)");
    p.Ucap = hash_bits < 40 ? std::min<uint64_t>(p.H_el, 1ULL << hash_bits) : p.H_el;
    // ---- which build: the bucket sort (rk_index_fast.inc) when the key fields fit, and then with TILE records as its product
    // (rk_index_tiles.inc) from RK_DIST_TILES_MIN_GENOMES genomes on -- the self join runs on rk_tile_kernel from its first launch --,
    // with slice records (rk_near_kernel, rk_dist_kernel) below
    // (round 5) The hash space is covered in RANGES (its top bits): one range per shard of a multi-GPU build
    // (rk_index_build_shard: this call builds the lists of ITS range only), and inside a shard as many passes as it takes to keep
    // a pass's keys within 2^15 buckets of ~1,536 -- a collection of any size takes the bucket sort, pass after pass on one
    // stream, the postings of a pass behind those of the pass before.
    p.shard_bits = shard_bits_of(n_shards);
    const uint64_t H_shard = H / n_shards + (n_shards > 1 ? H / (8ULL * n_shards) + 4096 : 0);   // (estimate: the hashes are spread evenly)
    // (a pass may fill its 2^15 buckets to ~2,600 keys on average: the LDS sort holds 4,096, and every extra pass reads all hashes again)
    p.pass_bits = 0;
    while (p.pass_bits < 8 && (H_shard >> p.pass_bits) > (2600ULL << kMaxBucketBits)) p.pass_bits++;
    if (k.pass_bits >= 0) p.pass_bits = k.pass_bits;
    p.range_bits = p.shard_bits + p.pass_bits;
    p.n_pass = 1u << p.pass_bits;
    p.eff_bits = hash_bits - p.range_bits;
    p.H_pass = p.range_bits ? (H_shard >> p.pass_bits) : H;
    p.H_el_shard = p.from_keys ? p.H_el : H / n_shards;
    // (at most kMaxBucketBits: a bigger collection gets fuller buckets, up to the LDS capacity -- beyond it the kernels raise the overflow flag)
    p.B = 1;
    while (p.B < p.eff_bits && p.B < kMaxBucketBits && ((p.H_pass + k.bucket_target - 1) / k.bucket_target) > (1ULL << p.B)) p.B++;
    if (p.from_keys) p.B = std::max(p.B, std::min(7, p.eff_bits));   // (the keys are a filtered source: the two-pass partition, >= 128 buckets)
    p.gb = genome_bits_of(N);
    p.rb = genome_bits_of(src.max_size);
    p.low_bits = p.eff_bits - p.B;
    // (64-bit hashes -- use64, e.g. K12 L3: 36 bits -- take the same path as long as the key fields fit: the kernels that read
    // the sketches are templated on the hash type, the bucket sort itself only ever sees the low bits)
    const bool fast_common = ctx->sw_index_fast && H && src.is_set && p.eff_bits >= 1 && p.B <= kMaxBucketBits && p.low_bits >= 0 && p.low_bits <= 31 && p.gb <= 31 && p.rb <= 31;
    p.slices_ok = fast_common && !p.range_bits && !p.no_self && H < (1ULL << 30) && p.low_bits + p.gb + p.rb <= 63;   // (slice records: one pass, offsets below 2^30)
    p.n_blocks = (N + 31) / 32;
    p.tiles_ok = fast_common && N >= 2 && p.n_blocks <= kTileMaxBlocks && p.low_bits + p.gb <= 63 && ctx->sw_index_tiles != 0;
    p.tiles_mode = p.tiles_ok && (p.range_bits || p.no_self || ctx->sw_index_tiles == 1 || N >= (uint32_t)ctx->sw_dist_tiles_min_genomes);
    if (n_shards > 1 && !p.tiles_mode)
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_index_build_shard needs set sketches of 2 .. %u genomes whose key fields fit the bucket sort "
                                                "(hash bits %d, %u shards)", kTileMaxBlocks * 32, hash_bits, n_shards);
    p.relabel = ctx->sw_index_relabel && src.is_set && N > 1 && H;
    p.two_streams = p.relabel && !k.one_stream;
    *out = p;
    return RK_OK;
}

// What the retries change from one bucket-sort attempt to the next.
struct RetryState {
    bool tiles_mode;               // the attempt emits tile records (false after the fallback: slice records)
    uint64_t keys_cap_retry = 0;   // keys of the fullest range pass, had they fit (the ranges of a real hash space are not equally full)
    uint64_t rec_cap_retry = 0;    // tile records the attempt before asked for, had they fit
};

// The decisions of ONE attempt: the plan + the retry state.
struct AttemptPlan {
    bool tiles_mode;
    bool sort_here;     // the tile sort runs in the build (a shard's records leave for the exchange: rk_index_join_shard sorts what arrives)
    bool part2;         // the two-pass partition: it needs six spare key bits and >= 128 buckets
    bool use_filter;    // a range pass partitions what k_range_filter kept of the hashes (RK_INDEX_FILTER=0: every kernel of the pass walks them all)
    bool small_wgs;     // k_part_coarse in several workgroups per chunk: they share its stretch through counters
    bool narrow;        // (hash_low, genome) fits 32 bits
    bool big_ok;        // buckets beyond the LDS sort (a hash shared by thousands of genomes) go to k_bucket_heavy: tile records, 32-bit sort keys
    uint32_t passes, nb, n_chunks;
    uint32_t part_chunks;   // rows of the count matrix
    uint32_t region_cap;
    int rb, range_bits;
    uint64_t keys_cap;  // what the key buffers of a pass hold
    uint64_t rec_cap;   // tile records the attempt has room for
};
int plan_attempt(rk_ctx *ctx, const BuildPlan &p, const BuildKnobs &k, const RetryState &rs, AttemptPlan *out)
{
    AttemptPlan a;
    a.tiles_mode = rs.tiles_mode;
    a.sort_here = a.tiles_mode && p.n_shards == 1;
    a.passes = a.tiles_mode ? p.n_pass : 1;
    a.rb = a.tiles_mode ? 0 : p.rb;   // (tile records: nobody needs an element's position inside its sketch)
    a.range_bits = a.tiles_mode ? p.range_bits : 0;
    a.nb = 1u << p.B;
    a.n_chunks = (uint32_t)((p.H_el + kPartChunk - 1) / kPartChunk);
    // what a pass may hold: exactly H without ranges; with ranges an estimate + slack (a pass that exceeds it raises the overflow
    // flag in k_part_starts and the kernels behind it stand still)
    // (from keys: the shard's exact key count -- a pass of it holds at most that many)
    const uint64_t pct = k.keys_cap_pct;
    a.keys_cap = p.from_keys ? std::max<uint64_t>(1, p.H_el)
               : a.range_bits ? std::min<uint64_t>(p.H, rs.keys_cap_retry ? rs.keys_cap_retry : p.H_pass * pct / 100 + (pct >= 100 ? (1u << 20) : 0)) : p.H;
    a.part2 = k.part2 && p.B >= 7 && p.low_bits + p.gb + a.rb <= 64 - (int)kFineBits;
    // (from keys: the keys ARE a filtered source -- of one pass as they arrived, of several through k_keys_pass_filter)
    a.use_filter = p.from_keys || (a.range_bits && a.part2 && p.eff_bits + p.gb <= 64 && k.filter);
    if (p.from_keys && !(a.part2 && a.tiles_mode && a.range_bits))
        return rk_fail(ctx, RK_ERR_UNSUPPORTED, "rk_index_build_shard_keys: the key fields do not fit the two-pass partition (hash bits %d, %d buckets, genome bits %d)",
                       p.hash_bits, p.B, p.gb);
    a.part_chunks = a.use_filter ? (uint32_t)((a.keys_cap + kPartChunk - 1) / kPartChunk) : a.n_chunks;
    a.small_wgs = (a.nb >> kFineBits) <= 128;
    a.narrow = p.low_bits + p.gb <= 32;
    a.big_ok = a.tiles_mode && a.narrow && ctx->sw_index_heavy;
    a.rec_cap = 0;
    a.region_cap = 0;
    if (a.tiles_mode) {
        // related lists write ~0.15-0.3 records per posting; chance collisions of a crowded hash space add H x lambda / 2
        // (lambda = postings per hash value: 500,000 genomes in 28 bits share every value twice over)
        const double lambda = p.hash_bits < 48 ? (double)p.H / (double)(1ULL << p.hash_bits) : 0.0;
        a.rec_cap = ctx->sw_tile_rec_cap ? ctx->sw_tile_rec_cap : rs.rec_cap_retry ? rs.rec_cap_retry : (uint64_t)((double)p.H_el_shard * (0.5 + 0.6 * lambda)) + 65536;
        a.rec_cap = std::min<uint64_t>(a.rec_cap, 0x7FFF0000ULL);
        a.region_cap = (uint32_t)((a.rec_cap + kRecRegions - 1) / kRecRegions);
        a.rec_cap = (uint64_t)a.region_cap * kRecRegions;
    }
    *out = a;
    return RK_OK;
}

// Everything the kernels expect zeroed, in one buffer and one fill (each fill is ~5 us on the stream; k_chunk_first, the first
// launch, does it): the result records, where the postings of each pass start, the cursors of the two-pass partition (per pass)
// and of the tile sort.  Offsets in 8-byte words; BuildResult, TileResult and pass_base[] lie back to back (the one read-back).
// rk_index_join_shard has the tile sort's part alone.
struct ZeroedLayout {
    size_t z_tres = 0, z_pass = 0, z_big = 0, z_filt = 0, z_hq = 0, z_cursor = 0, z_taken = 0, z_tcur = 0, z_bins = 0, z_end = 0;
    size_t w_cursor = 0, w_taken = 0;   // words per pass
    uint32_t n_blocks = 0;
    unsigned long long *base = nullptr;
    static ZeroedLayout of_build(uint32_t passes, bool part2, bool small_wgs, uint32_t nb, uint32_t n_chunks, bool sort_here, uint32_t n_blocks)
    {
        ZeroedLayout z;
        z.w_cursor = part2 ? (nb + 1) / 2 : 0;
        z.w_taken = part2 && small_wgs ? ((size_t)n_chunks * (nb >> kFineBits) + 1) / 2 : 0;
        z.z_tres = (sizeof(BuildResult) + 7) / 8;
        z.z_pass = z.z_tres + (sizeof(TileResult) + 7) / 8;
        z.z_big = z.z_pass + passes + 1;
        z.z_filt = z.z_big + (passes + 1) / 2;
        z.z_hq = z.z_filt + passes;
        z.z_cursor = z.z_hq + (passes + 1) / 2;
        z.z_taken = z.z_cursor + z.w_cursor * passes;
        z.tile_sort_at(z.z_taken + z.w_taken * passes, sort_here, n_blocks);
        return z;
    }
    static ZeroedLayout of_join(uint32_t n_blocks)
    {
        ZeroedLayout z;
        z.tile_sort_at((sizeof(TileResult) + 7) / 8, true, n_blocks);
        return z;
    }
    void tile_sort_at(size_t at, bool sort_here, uint32_t nbl)
    {
        n_blocks = nbl;
        z_tcur = at;
        z_bins = z_tcur + (sort_here ? (sizeof(TileCursors) + 7) / 8 : 0);
        z_end = z_bins + (sort_here ? (size_t)nbl + 1 : 0);   // bin counts (u32[n_blocks + 1]) + bin cursors (u32[n_blocks])
    }
    template <class T> T *at(size_t word) const { return reinterpret_cast<T *>(base + word); }
    BuildResult *res() const { return at<BuildResult>(0); }
    TileResult *tile_res() const { return at<TileResult>(z_tres); }
    unsigned long long *pass_base() const { return base + z_pass; }   // [passes + 1]: postings before pass p; the last one = all of them
    uint32_t *n_big(uint32_t pass) const { return at<uint32_t>(z_big) + pass; }
    unsigned long long *n_filtered(uint32_t pass) const { return base + z_filt + pass; }
    uint32_t *heavy_next(uint32_t pass) const { return at<uint32_t>(z_hq) + pass; }
    uint32_t *fine_cursor(uint32_t pass) const { return at<uint32_t>(z_cursor + w_cursor * pass); }
    uint32_t *seg_taken(uint32_t pass) const { return at<uint32_t>(z_taken + w_taken * pass); }
    TileCursors *tile_cursors() const { return at<TileCursors>(z_tcur); }
    uint32_t *bin_count() const { return at<uint32_t>(z_bins); }
    uint32_t *bin_cursor() const { return bin_count() + n_blocks + 1; }
};
