// rk_dist_tile.inc -- the all-vs-all self join over 32 x 32 tiles of the (genome, genome) matrix (included by rk_dist.hip
// inside its anonymous namespace).
//
// The row kernels (rk_near_kernel, rk_dist_kernel) read, for every (genome, hash) element, the list of LATER genomes that
// hold the hash: a species of C strains stores each of its lists C times, as C slices of up to C members, and a row's
// counts only stay in registers while its relatives fit a 32-column window.  That is the right shape for clades of ten and
// the wrong one for a species of hundreds of strains (measured: 10,000 genomes in species of 100 / 1,000 strains 1.4 / 4.2 ms
// against 0.033 ms in clades of ten).  Here the unit of work is the posting list itself, once:
//
//   A list's members (ascending internal genome ids) fall into aligned blocks of 32 ids.  For every pair of blocks (b <= w)
//   that the list touches it contributes ONE 8-byte record to tile (b, w): (bitmask of its members in block b, bitmask of its
//   members in block w) -- every cell (r in b, c in w) named by both masks gains one.  A clade hash shared by ten neighbouring
//   genomes is one record; a hash shared by all 1,000 strains of a species is 528 records standing for 499,500 cell
//   increments.  The records are sorted by tile (rk_tiles_build, lazily, once per index).
//
//   A tile is counted by one workgroup: lane = row (two records per wave step, one per half-wave), the record's column mask
//   is added to the lane's 32 column counters if the lane's row is in the row mask.  The 32 counters of a lane are
//   BIT-SLICED (plane k holds bit k of all 32): eight masks are first reduced by carry-save adders (three instructions
//   each) into one carry of weight 8, which ripples through the upper planes -- 3.3 vector instructions per record,
//   whatever the number of cells it names.  Counts move to LDS once per tile, cells are evaluated one per lane (FP64 as
//   in the row kernels), hits are staged in LDS.
//
//   Exactness without a fallback: a cell of tile (b, w) cannot count more than the tile has records, and a reportable
//   cell needs common >= min_jorc * denominator, where the denominator is at least the larger (jaccard) / the smaller
//   (containment) of the two sketches: a tile with fewer records than that bound for its smallest sketches is skipped --
//   the chance hashes shared by unrelated genomes never cost more than the look at the tile directory.  Every other tile
//   is counted exactly, so the result is the reference's for any width of cluster, any threshold, any sketch size.
//
// Sparse reports over set sketches only (a dense report names every cell; a repeated hash has a multiplicity a mask cannot
// carry): those stay with rk_dist_kernel.  Integer / bit work, bound by vector issue; no MFMA (a 0/1 co-occurrence product,
// deliberately kept as bit-sliced adds: 32 cells per lane-operation).

struct TileArgs {
    const unsigned long long *tile_key;   // b << 32 | w, ascending
    const unsigned long long *tile_start; // u64[n_tiles + 1] into contrib
    const uint32_t *blk_min;              // smallest non-empty sketch of every 32-id block (0xFFFFFFFF: none)
    const uint64_t *size_off;             // u64[n_ref + 1]: differences are the sketch sizes (internal order)
    const uint32_t *orig;                 // internal genome id -> the caller's (null: identity)
    const uint32_t *order;                // tile numbers by records per smallest sketch, descending (for this metric)
    const uint4 *dir;                     // the same order, one 32-byte entry per tile: {b, w, start lo, start hi} {records, denominator bound, 0, 0}
    unsigned long long n_tiles;
    uint32_t n_ref;
    uint32_t row_first, row_step, row_block;
    int metric, kmer_size;
    double max_dist, min_jorc;
    rk_hit *hits;
    unsigned long long cap;
    unsigned long long *n_hits;
    int debug;   // developer ablations (RK_TILE_DEBUG; results are then wrong by design): 1 no counting, 2 no evaluation, 4 no tile at all (directory look only), 8 no adds, 16 no merge / extraction, 32 / 64 only the first 512 / 256 tiles, 256 / 512 / 1024 the adder tree stops at a carry of weight 8 / 16 / 32, 4096 no hit-count atomic
};

constexpr unsigned long long kTileSrowPerTile = 2000ULL;   // tile_launch_shape: records per launched tile from which a short launch takes the scalar row masks
constexpr int kTilePlanes = 11;          // a lane adds at most 2,040 records before its planes move to LDS

// carry-save adder over bit planes: (a, b, c) -> sum in `a`, carry returned: TWO v_bitop3_b32 (three-input truth tables:
// parity 0x96, majority 0xE8).  History: an inline-asm xor / bfi / xor "measured no different" from what the compiler made of
// plain expressions while extraction and latency bound the kernel; once they did not, the asm's three instructions per adder
// plus an s_nop after most of them (opaque to the scheduler: 67 in a step of 128 records) were a quarter of the vector work,
// and plain expressions compile to a MIX (a ^ b shared, then bitop3: 509 instructions per step instead of 394).  The builtin
// gives exactly the two.
__device__ inline uint32_t csa(uint32_t &a, uint32_t b, uint32_t c)
{
    const uint32_t carry = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
    a = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
    return carry;
}
// plane += carry: returns the carry out
__device__ inline uint32_t ripple(uint32_t &p, uint32_t carry)
{
    const uint32_t c2 = p & carry;
    p ^= carry;
    return c2;
}

// SROW: the row masks come as 64-bit scalars and select with one v_cndmask (short launches); else both masks pass through LDS
// and a lane tests its row with v_bfe_i32 + v_and (long launches: a stream of row masks through the scalar caches does not scale)
template <uint32_t kTileThreads, bool SROW>
__global__ __launch_bounds__(kTileThreads, kTileThreads == 256 ? 6 : 4) void rk_tile_kernel(TileArgs a, const uint2 *__restrict__ contrib, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ cols)
{
    constexpr uint32_t kTileWaves = kTileThreads / 64;
    // a wave's share of a tile's records is rounded up to this many.  Eight and sixteen waves (launches of one round of
    // workgroups: a tile's chain is the launch) take EVEN shares in whole groups of 16 records: whole 128-record steps left
    // seven waves five steps and the eighth two on a tile of 4,728 records, and three of eight waves idle on one of 1,194.
    // Four waves (launches of several rounds, bound by vector issue) keep whole steps: there a chain's length buys nothing and
    // a partial step costs more instructions per record (measured with groups of 16: 50,000 genomes 0.0629 -> 0.0642 ms,
    // species of 1,000 strains 0.0479 -> 0.0482; DESIGN 4.3c)
    constexpr uint32_t kTileShare = kTileWaves >= 8 ? 16u : 128u;
    // hits are staged in the LDS that held the tile's records while it was counted (flushed when a round of cells may not
    // fit, and at the end of every tile)
    constexpr uint32_t kTileStage = (uint32_t)(8 * kTileThreads * sizeof(uint2) / sizeof(rk_hit));
    static_assert(kTileStage >= kTileThreads + 64, "a round of cells fits the stage");
    __shared__ uint32_t cnt[32 * 32];            // [col][row]
    __shared__ __attribute__((aligned(16))) uint2 recs[8 * kTileThreads];     // the chunk of tile records being counted
    rk_hit *stage = reinterpret_cast<rk_hit *>(recs);
    __shared__ uint32_t s_cursor;
    __shared__ unsigned long long s_base;
    __shared__ uint32_t rsize[32], csize[32];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t half = lane >> 5, row = lane & 31;

    // ---- this workgroup's tile: the blockIdx-th of the directory ordered by records per smallest sketch, descending (the
    // launch covers the prefix that can hold a reportable cell, by a table of the host; the exact test is made here)
    const uint4 d0 = a.dir[2 * (size_t)blockIdx.x], d1 = a.dir[2 * (size_t)blockIdx.x + 1];   // (one access: k_tile_dir)
    const uint32_t b = d0.x, w = d0.y;
    const unsigned long long s0 = (unsigned long long)d0.z | ((unsigned long long)d0.w << 32), s1 = s0 + d1.x;
    {
        const uint32_t lb = d1.y;   // lower bound of any cell's denominator: the larger (jaccard) / the smaller (containment) of the blocks' smallest sketches
        bool take = (double)(s1 - s0) >= a.min_jorc * (double)lb;
        if (take && a.row_step > 1) {   // a pair belongs to the shard of its row: any row of the block in this shard?
            bool mine = false;
            const uint32_t r0 = b * 32, r1 = min(a.n_ref, r0 + 32);
            for (uint32_t blk = r0 / a.row_block; blk <= (r1 - 1) / a.row_block; blk++) mine |= blk % a.row_step == a.row_first;
            take = mine;
        }
        if (!take || (a.debug & 4) || ((a.debug & 32) && blockIdx.x >= 512) || ((a.debug & 64) && blockIdx.x >= 256)) return;   // (uniform)
    }
    for (uint32_t i = tid; i < 32 * 32; i += kTileThreads) cnt[i] = 0;
    if (tid == 0) s_cursor = 0;
    __syncthreads();

    auto flush_stage = [&]() {   // (all threads)
        __syncthreads();
        const uint32_t n_st = min(s_cursor, kTileStage);
        if (n_st) {
            // (RK_TILE_DEBUG & 4096: no atomic -- the hits land anywhere; what the returning device-scope atomic of every tile costs:
            // 10,000 genomes 0.0184 -> 0.0160 ms, species of 1,000 strains 0.050 -> 0.041, 50,000 genomes 0.061 -> 0.052)
            if (tid == 0) s_base = (a.debug & 4096) ? (unsigned long long)blockIdx.x * 128ULL : atomicAdd(a.n_hits, (unsigned long long)n_st);
            __syncthreads();
            const unsigned long long at0 = s_base;
            const unsigned long long *src = reinterpret_cast<const unsigned long long *>(stage);
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.hits);
            constexpr uint32_t kW = sizeof(rk_hit) / 8;
            for (uint32_t i = tid; i < n_st * kW; i += kTileThreads)
                if (at0 + i / kW < a.cap) dst[at0 * kW + i] = src[i];
        }
        __syncthreads();
        if (tid == 0) s_cursor = 0;
        __syncthreads();
    };

    {
        if (tid < 64) {   // sketch sizes of the tile's rows and columns
            const uint32_t g = (tid < 32 ? b : w) * 32 + (tid & 31);
            const uint32_t sz = g < a.n_ref ? (uint32_t)(a.size_off[g + 1] - a.size_off[g]) : 0u;
            if (tid < 32) rsize[tid] = sz; else csize[tid - 32] = sz;
        }
        // ---- counting.  The tile's records pass through LDS in chunks of 8 per thread: coalesced global loads (the next
        // chunk's are in flight while this one is counted), then every wave counts its quarter of the chunk, two records per
        // step (one per half-wave, read from LDS as a broadcast).  Records behind the tile's end are stored as zeros.
        uint32_t p[kTilePlanes + 1];   // (the extra plane: the sum of the two half-waves)
#pragma unroll
        for (int k = 0; k <= kTilePlanes; k++) p[k] = 0;
        uint32_t steps = 0;
        auto to_lds = [&]() {
            // the other half-wave's counters of my row (lane ^ 32) are added in bit-sliced form: 11 + 11 planes -> 12 ...
            uint32_t carry = 0;
#pragma unroll
            for (int k = 0; k < kTilePlanes; k++) {
                const uint32_t o = (uint32_t)__shfl_xor((int)p[k], 32);
                const uint32_t u = p[k] ^ o;
                const uint32_t c2 = (p[k] & o) | (u & carry);
                p[k] = u ^ carry;
                carry = c2;
            }
            p[kTilePlanes] = carry;
            // ... and each half-wave moves 16 of the 32 columns to LDS
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k <= kTilePlanes; k++) any |= p[k];
            const uint32_t occupied = wave_or(any);   // uniform: columns some lane counted
            uint32_t occ2 = (occupied | (occupied >> 16)) & 0xFFFFu;   // column c of half 0 and column c + 16 of half 1 together
            while (occ2) {
                const int c = __builtin_ctz(occ2) + 16 * (int)half;
                occ2 &= occ2 - 1;
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k <= kTilePlanes; k++) v |= ((p[k] >> c) & 1u) << k;
                if (v) atomicAdd(&cnt[c * 32 + row], v);
            }
#pragma unroll
            for (int k = 0; k <= kTilePlanes; k++) p[k] = 0;
            steps = 0;
        };
        auto add8 = [&](const uint32_t (&m)[8]) {
            // eight masks -> one carry of weight 8 (Harley-Seal): ones = p[0], twos = p[1], fours = p[2]
            const uint32_t t2a = csa(p[0], m[0], m[1]);
            const uint32_t t2b = csa(p[0], m[2], m[3]);
            const uint32_t t4a = csa(p[1], t2a, t2b);
            const uint32_t t2c = csa(p[0], m[4], m[5]);
            const uint32_t t2d = csa(p[0], m[6], m[7]);
            const uint32_t t4b = csa(p[1], t2c, t2d);
            uint32_t carry = csa(p[2], t4a, t4b);
#pragma unroll
            for (int k = 3; k < kTilePlanes; k++) carry = ripple(p[k], carry);
            steps += 8;
            if (steps >= 1984) to_lds();   // (uniform: before a lane's count can pass the 2,047 of eleven planes -- the next step adds at most 64)
        };
        // Harley-Seal above the eights: two groups of eight masks leave two carries of weight 8 that meet in one more adder
        // (plane 3) -> ONE carry of weight 16; two of those meet in plane 4 -> one carry of weight 32 that ripples through planes
        // 5..10: 105 instructions per 32 masks instead of 148 with a ripple per eight (no gain while extraction and latency
        // bound the kernel -- now that 50,000 genomes keep the vector pipes 93 % busy it is what the time goes into)
        auto carry16 = [&](const uint32_t (&ma)[8], const uint32_t (&mb)[8]) -> uint32_t {
            const uint32_t a2a = csa(p[0], ma[0], ma[1]);
            const uint32_t a2b = csa(p[0], ma[2], ma[3]);
            const uint32_t a4a = csa(p[1], a2a, a2b);
            const uint32_t a2c = csa(p[0], ma[4], ma[5]);
            const uint32_t a2d = csa(p[0], ma[6], ma[7]);
            const uint32_t a4b = csa(p[1], a2c, a2d);
            const uint32_t c8a = csa(p[2], a4a, a4b);
            const uint32_t b2a = csa(p[0], mb[0], mb[1]);
            const uint32_t b2b = csa(p[0], mb[2], mb[3]);
            const uint32_t b4a = csa(p[1], b2a, b2b);
            const uint32_t b2c = csa(p[0], mb[4], mb[5]);
            const uint32_t b2d = csa(p[0], mb[6], mb[7]);
            const uint32_t b4b = csa(p[1], b2c, b2d);
            const uint32_t c8b = csa(p[2], b4a, b4b);
            return csa(p[3], c8a, c8b);
        };
        auto add16 = [&](const uint32_t (&ma)[8], const uint32_t (&mb)[8]) {
            uint32_t carry = carry16(ma, mb);
#pragma unroll
            for (int k = 4; k < kTilePlanes; k++) carry = ripple(p[k], carry);
            steps += 16;
            if (steps >= 1984) to_lds();   // (uniform)
        };
        if (!(a.debug & 1)) {
            if constexpr (SROW) {
                // every wave streams its own share of the tile's records, 128 at a time.  The records are kept split: the COLUMN masks
                // pass through LDS (two coalesced 4-byte loads per lane, three batches in flight, stored de-interleaved into the wave's
                // own slot -- even records for half-wave 0, odd ones for half-wave 1 -- and read back 4 at a time as broadcasts; no
                // workgroup barrier: a wave's LDS operations execute in order); the ROW masks never touch a vector register: two
                // neighbouring records' row masks are one aligned 64-bit scalar (s_load: the wave's position is uniform) that IS the
                // lane mask of a v_cndmask -- lane = row, half-wave 0 takes the even record, half-wave 1 the odd one -- so a record
                // costs ONE vector instruction before the adders (v_bfe_i32 + v_and before: 128 of a step's 329).  Column masks behind
                // the wave's share are stored as zeros (whatever row mask they meet then selects nothing).
                constexpr int kDepth = 3;
                // (positions inside the tile in 32 bits: a tile has fewer than 2^32 records -- the directory entry says so)
                const unsigned long long slot0 = (unsigned long long)d1.z | ((unsigned long long)d1.w << 32);   // the tile's first slot in the split arrays: even
                const unsigned long long *__restrict__ tile_rows = reinterpret_cast<const unsigned long long *>(rows + slot0);
                const uint32_t n_rec = d1.x;
                const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
                // a wave's share (kTileShare above): it starts on an even record, so the pairs of row masks stay aligned, and its
                // tail takes the partial-step paths below.  Furthest slot read: below w0 + n_sub * 128 <= w1 + 127 <= n_rec + 127,
                // inside the 256 slots that pad the arrays.  (to_lds() counts per lane, whatever the share.)
                const uint32_t per = ((n_rec + kTileWaves - 1) / kTileWaves + kTileShare - 1u) & ~(kTileShare - 1u);
                const uint32_t w0 = min(n_rec, wave_u * per), w1 = min(n_rec, w0 + per);
                const uint32_t n_sub = (w1 - w0 + 127u) / 128u;
                const uint32_t *__restrict__ tile_cols = cols + slot0;   // (the column masks in the same padded slots)
                uint32_t *mine = reinterpret_cast<uint32_t *>(recs + wave * 512);   // 4 slots x 128 column masks (the rest of the wave's region: the planes at the end)
                uint32_t in0[kDepth], in1[kDepth];
                auto request = [&](uint32_t sub, int slot) {
                    const uint32_t at = w0 + sub * 128u + lane;   // (the arrays are padded by 256 slots: no clamp; masked when stored)
                    in0[slot] = tile_cols[at];
                    in1[slot] = tile_cols[at + 64u];
                };
                // where a record's column mask goes inside a slot: even records to [0, 64), odd ones to [64, 128)
                const uint32_t put0 = (lane & 1u) * 64u + (lane >> 1), put1 = put0 + 32u;
    #pragma unroll
                for (int d = 0; d < kDepth; d++)
                    if ((uint32_t)d < n_sub) request((uint32_t)d, d);
                for (uint32_t sub0 = 0; sub0 < n_sub; sub0 += kDepth) {
    #pragma unroll
                    for (int d = 0; d < kDepth; d++) {
                        const uint32_t sub = sub0 + d;
                        if (sub >= n_sub) break;   // (uniform)
                        const uint32_t at = w0 + sub * 128u + lane;
                        uint32_t *slot = mine + (sub & 3u) * 128;
                        slot[put0] = at < w1 ? in0[d] : 0u;
                        slot[put1] = at + 64u < w1 ? in1[d] : 0u;
                        if (sub + kDepth < n_sub) request(sub + kDepth, d);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        const uint32_t n_here = min(128u, w1 - (w0 + sub * 128u));
                        const uint4 *rd = reinterpret_cast<const uint4 *>(slot + 64 * half);   // my half-wave's 64 column masks
                        const unsigned long long *pairs = tile_rows + ((w0 + sub * 128u) >> 1);   // (uniform) 64 pairs of row masks
                        // (reading the next group's records while this one is added was tried twice: 10,000 genomes 0.0325 -> 0.037 ms and,
                        // with the 16-byte reads, 0.0305 -> 0.0364; 50,000 0.088 -> 0.106: the sixteen extra registers and the moves cost
                        // more than the LDS latency they hide, also where occupancy does not matter)
                        const uint32_t n_groups = min(8u, (n_here + 15) / 16);   // (uniform) a group: 8 pairs of neighbouring records
                        auto masks_sel = [&](uint32_t g, const unsigned long long *sel, uint32_t (&m)[8]) {
                            const uint4 r0 = rd[2 * g], r1 = rd[2 * g + 1];
                            const uint32_t y[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    #pragma unroll
                            for (int j = 0; j < 8; j++)
                                asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(m[j]) : "v"(y[j]), "s"(sel[j]));
                        };
                        auto masks = [&](uint32_t g, uint32_t (&m)[8]) {
                            unsigned long long sel[8];
    #pragma unroll
                            for (int j = 0; j < 8; j++) sel[j] = pairs[8 * g + j];
                            const uint4 r0 = rd[2 * g], r1 = rd[2 * g + 1];
                            const uint32_t y[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    #pragma unroll
                            for (int j = 0; j < 8; j++)   // the column mask where the lane's row is named (lane mask = the pair's two row masks)
                                asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(m[j]) : "v"(y[j]), "s"(sel[j]));
                        };
                        uint32_t g = 0;
                        auto carry32 = [&](uint32_t g0) -> uint32_t {   // groups g0 .. g0 + 3
                            // (the row masks of all four groups requested at once -- 64 scalar registers --: a scalar load that misses
                            // costs its latency once per 64 records instead of once per 16)
                            unsigned long long sel[32];
    #pragma unroll
                            for (int j = 0; j < 32; j++) sel[j] = pairs[8 * g0 + j];
                            uint32_t ma[8], mb[8];
                            masks_sel(g0, sel, ma);
                            masks_sel(g0 + 1, sel + 8, mb);
                            const uint32_t c16a = carry16(ma, mb);
                            masks_sel(g0 + 2, sel + 16, ma);
                            masks_sel(g0 + 3, sel + 24, mb);
                            const uint32_t c16b = carry16(ma, mb);
                            return csa(p[4], c16a, c16b);
                        };
                        if (n_groups == 8 && !(a.debug & (256 | 512 | 1024))) {   // a full step: one carry of weight 64
                            const uint32_t c32a = carry32(0);
                            const uint32_t c32b = carry32(4);
                            uint32_t carry = csa(p[5], c32a, c32b);
    #pragma unroll
                            for (int k = 6; k < kTilePlanes; k++) carry = ripple(p[k], carry);
                            steps += 64;
                            if (steps >= 1984) to_lds();   // (uniform)
                            g = 8;
                        }
                        for (; g + 3 < n_groups && !(a.debug & (256 | 512)); g += 4) {
                            uint32_t carry = carry32(g);
    #pragma unroll
                            for (int k = 5; k < kTilePlanes; k++) carry = ripple(p[k], carry);
                            steps += 32;
                            if (steps >= 1984) to_lds();   // (uniform)
                        }
                        for (; g + 1 < n_groups && !(a.debug & 256); g += 2) {
                            uint32_t ma[8], mb[8];
                            masks(g, ma);
                            masks(g + 1, mb);
                            if (a.debug & 8) { p[0] |= ma[0] | ma[1] | ma[2] | ma[3] | ma[4] | ma[5] | ma[6] | ma[7] | mb[0] | mb[7]; continue; }
                            add16(ma, mb);
                        }
                        for (; g < n_groups; g++) {
                            uint32_t m[8];
                            masks(g, m);
                            if (a.debug & 8) { p[0] |= m[0] | m[1] | m[2] | m[3] | m[4] | m[5] | m[6] | m[7]; continue; }
                            add8(m);
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            } else {
                // every wave streams its own share of the tile's records, 128 at a time: two coalesced loads (lane i: records i
                // and 64 + i; three batches in flight), a store into the wave's own quarter of `recs` (four slots of 128
                // records, no workgroup barrier: a wave's LDS operations execute in order), then 8 groups of 16 records read
                // back as broadcasts.  Records behind the wave's share are stored as zeros.
                constexpr int kDepth = 3;
                // (positions inside the tile in 32 bits: a tile has fewer than 2^32 records -- the directory entry says so)
                const uint2 *__restrict__ tile = contrib + s0;
                const uint32_t n_rec = d1.x;
                // (a wave's share: kTileShare above; loads are clamped to the tile: nothing is read behind it)
                const uint32_t per = ((n_rec + kTileWaves - 1) / kTileWaves + kTileShare - 1u) & ~(kTileShare - 1u);
                const uint32_t w0 = min(n_rec, wave * per), w1 = min(n_rec, w0 + per);
                const uint32_t n_sub = (w1 - w0 + 127u) / 128u;
                uint2 *mine = recs + wave * 512;   // 4 slots x 128 records
                uint2 in0[kDepth], in1[kDepth];
                auto request = [&](uint32_t sub, int slot) {
                    const uint32_t at = w0 + sub * 128u + lane;
                    in0[slot] = tile[min(at, n_rec - 1u)];        // (clamped, masked when stored: no branch per load)
                    in1[slot] = tile[min(at + 64u, n_rec - 1u)];
                };
    #pragma unroll
                for (int d = 0; d < kDepth; d++)
                    if ((uint32_t)d < n_sub) request((uint32_t)d, d);
                for (uint32_t sub0 = 0; sub0 < n_sub; sub0 += kDepth) {
    #pragma unroll
                    for (int d = 0; d < kDepth; d++) {
                        const uint32_t sub = sub0 + d;
                        if (sub >= n_sub) break;   // (uniform)
                        const uint32_t at = w0 + sub * 128u + lane;
                        uint2 *slot = mine + (sub & 3u) * 128;
                        slot[lane] = at < w1 ? in0[d] : make_uint2(0, 0);
                        slot[64 + lane] = at + 64u < w1 ? in1[d] : make_uint2(0, 0);
                        if (sub + kDepth < n_sub) request(sub + kDepth, d);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        const uint32_t n_here = min(128u, w1 - (w0 + sub * 128u));
                        // half-wave 0 counts records 0 .. 63 of the slot, half-wave 1 records 64 .. 127: two neighbouring records per
                        // 16-byte LDS read (a broadcast inside the half-wave)
                        const uint4 *rd = reinterpret_cast<const uint4 *>(slot + 64 * half);
                        // (reading the next group's records while this one is added was tried twice: 10,000 genomes 0.0325 -> 0.037 ms and,
                        // with the 16-byte reads, 0.0305 -> 0.0364; 50,000 0.088 -> 0.106: the sixteen extra registers and the moves cost
                        // more than the LDS latency they hide, also where occupancy does not matter)
                        const uint32_t n_groups = min(8u, (n_here + 7) / 8);   // (uniform; a slot's first 64 records fill up first)
                        auto masks = [&](uint32_t g, uint32_t (&m)[8]) {
    #pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const uint4 r = rd[4 * g + j];
                                m[2 * j] = (uint32_t)__builtin_amdgcn_sbfe((int)r.x, row, 1) & r.y;   // the column mask if my row is named
                                m[2 * j + 1] = (uint32_t)__builtin_amdgcn_sbfe((int)r.z, row, 1) & r.w;
                            }
                        };
                        uint32_t g = 0;
                        auto carry32 = [&](uint32_t g0) -> uint32_t {   // groups g0 .. g0 + 3
                            uint32_t ma[8], mb[8];
                            masks(g0, ma);
                            masks(g0 + 1, mb);
                            const uint32_t c16a = carry16(ma, mb);
                            masks(g0 + 2, ma);
                            masks(g0 + 3, mb);
                            const uint32_t c16b = carry16(ma, mb);
                            return csa(p[4], c16a, c16b);
                        };
                        if (n_groups == 8 && !(a.debug & (256 | 512 | 1024))) {   // a full step: one carry of weight 64
                            const uint32_t c32a = carry32(0);
                            const uint32_t c32b = carry32(4);
                            uint32_t carry = csa(p[5], c32a, c32b);
    #pragma unroll
                            for (int k = 6; k < kTilePlanes; k++) carry = ripple(p[k], carry);
                            steps += 64;
                            if (steps >= 1984) to_lds();   // (uniform)
                            g = 8;
                        }
                        for (; g + 3 < n_groups && !(a.debug & (256 | 512)); g += 4) {
                            uint32_t carry = carry32(g);
    #pragma unroll
                            for (int k = 5; k < kTilePlanes; k++) carry = ripple(p[k], carry);
                            steps += 32;
                            if (steps >= 1984) to_lds();   // (uniform)
                        }
                        for (; g + 1 < n_groups && !(a.debug & 256); g += 2) {
                            uint32_t ma[8], mb[8];
                            masks(g, ma);
                            masks(g + 1, mb);
                            if (a.debug & 8) { p[0] |= ma[0] | ma[1] | ma[2] | ma[3] | ma[4] | ma[5] | ma[6] | ma[7] | mb[0] | mb[7]; continue; }
                            add16(ma, mb);
                        }
                        for (; g < n_groups; g++) {
                            uint32_t m[8];
                            masks(g, m);
                            if (a.debug & 8) { p[0] |= m[0] | m[1] | m[2] | m[3] | m[4] | m[5] | m[6] | m[7]; continue; }
                            add8(m);
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
        }
        // ---- (round 4, late) the end of the tile: the waves' counters are ADDED IN BIT-SLICED FORM -- through the LDS that held
        // the records, pairwise, log2(waves) rounds of one 16-plane ripple add -- and every wave then extracts only its share
        // of the 32 columns from the total (before: every wave extracted all columns of its own planes with LDS atomics:
        // ~700 vector instructions per wave and tile, as many as the counting itself on a species of 1,000 strains)
        if (!(a.debug & 16)) {
            constexpr int kAll = 16;   // planes of the total: 2 half-waves x 16 waves x 2,047 < 2^16
            uint32_t q[kAll];
            {   // the other half-wave's counters of my row (lane ^ 32)
                uint32_t carry = 0;
#pragma unroll
                for (int k = 0; k < kTilePlanes; k++) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)p[k], 32);
                    const uint32_t u = p[k] ^ o;
                    q[k] = u ^ carry;
                    carry = (p[k] & o) | (u & carry);
                }
                q[kTilePlanes] = carry;
#pragma unroll
                for (int k = kTilePlanes + 1; k < kAll; k++) q[k] = 0;
            }
            uint32_t *all_planes = reinterpret_cast<uint32_t *>(recs);   // a wave's region: 512 records = 1,024 words >= 16 planes x 32 rows
            uint32_t *my_planes = all_planes + wave * 1024;
            auto publish = [&]() {
                if (lane < 32) {
#pragma unroll
                    for (int k = 0; k < kAll; k++) my_planes[k * 32 + row] = q[k];
                }
            };
            if (kTileWaves > 1) publish();
            __syncthreads();
#pragma unroll
            for (uint32_t stride = 1; stride < kTileWaves; stride <<= 1) {
                if ((wave & (2 * stride - 1)) == 0) {   // (uniform per wave)
                    const uint32_t *theirs = all_planes + (wave + stride) * 1024;
                    uint32_t carry = 0;
#pragma unroll
                    for (int k = 0; k < kAll; k++) {
                        const uint32_t o = theirs[k * 32 + row];
                        const uint32_t u = q[k] ^ o;
                        const uint32_t c2 = (q[k] & o) | (u & carry);
                        q[k] = u ^ carry;
                        carry = c2;
                    }
                    publish();   // (the next round's partner reads it; after the last round: the total, in wave 0's region)
                }
                __syncthreads();
            }
            if (kTileWaves > 1) {
#pragma unroll
                for (int k = 0; k < kAll; k++) q[k] = all_planes[k * 32 + row];
            }
            constexpr uint32_t kColsPerHalf = 16 / kTileWaves;
#pragma unroll
            for (uint32_t i = 0; i < kColsPerHalf; i++) {
                const uint32_t c = wave * (32 / kTileWaves) + half * kColsPerHalf + i;
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < kAll; k++) v |= ((q[k] >> c) & 1u) << k;
                if (v) cnt[c * 32 + row] += v;   // (every cell belongs to one lane; a mid-tile flush may have left a count)
            }
        }
        __syncthreads();
        // ---- evaluation: one cell per lane and round.  A tile off the diagonal has 1,024 cells.  In a DIAGONAL tile (b == w) only
        // the 496 cells with col > row pass `gcol > grow` below: they are numbered by rk_tile_tri_cell (rk_tile_cells.h; a wave's
        // reads of cnt meet 2-way at most) and take ceil(496 / threads) rounds -- one instead of two at 512 threads --, the
        // lanes from 496 on hold no cell.  The diagonal and the lower triangle of cnt are never read and need no clearing here:
        // a workgroup counts ONE tile, and the whole matrix is zeroed where it always was, at the tile's start.
        const bool diag = b == w;   // (uniform)
        const uint32_t n_rounds = diag ? (kTileTriCells + kTileThreads - 1) / kTileThreads : 1024 / kTileThreads;
        for (uint32_t round = 0; round < n_rounds; round++) {
            if (s_cursor + kTileThreads > kTileStage) flush_stage();   // (uniform: s_cursor only changes between barriers)
            uint32_t ci = round * kTileThreads + tid;
            uint32_t col = ci >> 5, r = ci & 31;
            bool cell = true;
            if (diag) {
                cell = rk_tile_tri_cell(ci, r, col);
                ci = cell ? col * 32 + r : 0u;
            }
            uint32_t common = 0;
            if (cell) {
                common = cnt[ci];
                cnt[ci] = 0;
            }
            const uint32_t grow = b * 32 + r, gcol = w * 32 + col;
            bool ok = common != 0 && gcol > grow && gcol < a.n_ref && !(a.debug & 2);
            if (ok && a.row_step > 1) ok = (grow / a.row_block) % a.row_step == a.row_first;
            if (ok) {
                const int size0 = (int)rsize[r], size1 = (int)csize[col];   // src/dist.cpp:215-216
                const int denom = a.metric ? min(size0, size1) : size0 + size1 - (int)common;
                if ((double)common >= a.min_jorc * (double)denom) {   // exact-safe reject before the FP64 divide + log
                    const JorcDist jd = rk_distance((int)common, size0, size1, a.metric, a.kmer_size);
                    if (jd.dist < a.max_dist) {   // src/dist.cpp:232
                        uint32_t out_row = grow, out_col = gcol;
                        if (a.orig) {   // the caller's genome indices, smaller one as the row (src/dist.cpp:207)
                            out_row = a.orig[grow];
                            out_col = a.orig[gcol];
                        }
                        const bool flip = out_row > out_col;
                        rk_hit hrec;
                        hrec.row = flip ? out_col : out_row;
                        hrec.col = flip ? out_row : out_col;
                        hrec.common = (int)common;
                        hrec.size0 = flip ? size1 : size0;
                        hrec.size1 = flip ? size0 : size1;
                        hrec.pad_ = 0;
                        hrec.jorc = jd.jorc;
                        hrec.dist = jd.dist;
                        stage[atomicAdd(&s_cursor, 1u)] = hrec;   // (a round stages at most 256 hits: room was made above)
                    }
                }
            }
            __syncthreads();
        }
        flush_stage();
    }
}

// launch shape of the tile kernel for these options: workgroups (= tiles of the density-ordered directory that may hold a
// reportable cell, by the host's table; the kernel tests exactly) and threads per workgroup
struct TileShape { unsigned long long grid = 0; int threads = 256; bool srow = false; };
TileShape tile_launch_shape(const rk_index *idx, const rk_dist_opts *o, double min_jorc)
{
    const int metric = o->metric != 0;
    unsigned long long grid = idx->n_tiles;
    if (min_jorc > 0.0) {
        const double kk = ceil(-8.0 * log2(min_jorc));
        if (kk < (double)kTileTable) grid = idx->tile_prefix[metric][kk < 0.0 ? 0 : (int)kk];
    }
    if (getenv("RK_TILE_ALL")) grid = idx->n_tiles;   // (developer: every tile gets a workgroup)
    // waves per tile: a tile is a chain of ~300 records per wave at four waves; when the launch has few tiles for the chip
    // (10,000 genomes: ~560) eight waves share a tile (measured, 10,000 genomes in clades of 10 / 100: 0.038 / 0.048 ms with
    // four, 0.033 / 0.037 with eight; 50,000 genomes / species of 1,000: 0.088 / 0.070 with four, 0.098 / 0.085 with eight)
    const uint32_t row_step = o->row_step ? o->row_step : 1;
    int threads = grid / row_step < 1500 ? 512 : 256;
    if (grid / row_step < 150) threads = 1024;   // (a 1/8 row shard of 10,000 genomes, ~70 tiles: 0.036 ms with 512 threads, 0.024 with 1,024)
    if (getenv("RK_TILE_THREADS")) threads = atoi(getenv("RK_TILE_THREADS"));
    if (threads != 512 && threads != 1024) threads = 256;
    // row masks as scalars (SROW) for short launches (one round of workgroups: 512 / 1,024 threads) whose tiles hold a few
    // steps of records per wave -- there the vector instructions saved are time saved (10,000 genomes in clades of ten: 0.0214
    // -> 0.0185 ms, 4,000: 0.0152 -> 0.0144, a 1/8 row shard 0.0141 -> 0.0127); where a wave has one or two steps (species of
    // 100 strains: 0.0285 -> 0.0316) or the launch keeps the chip busy for several rounds (50,000 genomes: 0.0657 -> 0.070) the
    // scalar loads cost more than they save: their latency has nothing to hide behind, and a stream of row masks through the
    // scalar caches does not scale
    bool srow = threads >= 512 && grid && idx->n_tile_records >= kTileSrowPerTile * grid && idx->d_tile_rows;   // (d_tile_rows: the split copy exists)
    if (getenv("RK_TILE_SROW")) srow = atoi(getenv("RK_TILE_SROW")) != 0 && idx->d_tile_rows;
    return TileShape{grid, threads, srow};
}

int launch_tiles(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, double min_jorc, const TileShape &shape, rk_hit *hits_dev, uint64_t cap,
                 unsigned long long *n_hits_dev, hipStream_t stream)
{
    if (!idx->n_tiles) return RK_OK;
    TileArgs a;
    a.tile_key = idx->d_tile_key;
    a.tile_start = idx->d_tile_start;
    a.blk_min = idx->d_blk_min;
    a.size_off = idx->d_src_off;
    a.orig = idx->relabeled ? idx->d_orig : nullptr;
    a.n_tiles = idx->n_tiles;
    a.n_ref = idx->n_ref;
    a.order = idx->d_tile_order[o->metric != 0];
    a.dir = idx->d_tile_dir[o->metric != 0];
    const RowShard rows(o, idx->n_ref, 0);
    a.row_step = rows.row_step;
    a.row_first = rows.row_first;
    a.row_block = rows.row_block;
    a.metric = o->metric != 0;
    a.kmer_size = o->kmer_size;
    a.max_dist = o->max_dist;
    a.min_jorc = min_jorc;
    a.hits = hits_dev;
    a.cap = cap;
    a.n_hits = n_hits_dev;
    a.debug = getenv("RK_TILE_DEBUG") ? atoi(getenv("RK_TILE_DEBUG")) : 0;
    if (!shape.grid) return RK_OK;
    if (shape.grid > 0x7FFFFFFFULL) return rk_fail(ctx, RK_ERR_UNSUPPORTED, "too many tiles for one launch (%llu)", (unsigned long long)idx->n_tiles);
#define RK_TILE_LAUNCH(T)                                                                                                              \
    do {                                                                                                                               \
        if (shape.srow) hipLaunchKernelGGL((rk_tile_kernel<T, true>), dim3((unsigned)shape.grid), dim3(T), 0, stream, a, (const uint2 *)idx->d_tile_contrib, (const uint32_t *)idx->d_tile_rows, (const uint32_t *)idx->d_tile_cols); \
        else hipLaunchKernelGGL((rk_tile_kernel<T, false>), dim3((unsigned)shape.grid), dim3(T), 0, stream, a, (const uint2 *)idx->d_tile_contrib, (const uint32_t *)idx->d_tile_rows, (const uint32_t *)idx->d_tile_cols); \
    } while (0)
    if (shape.threads == 512)
        RK_TILE_LAUNCH(512);
    else if (shape.threads == 1024)
        RK_TILE_LAUNCH(1024);
    else
        RK_TILE_LAUNCH(256);
#undef RK_TILE_LAUNCH
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}
