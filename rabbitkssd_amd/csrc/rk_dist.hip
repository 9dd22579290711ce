// rk_dist.hip -- intersection counting through the inverted index + distance epilogue.
// Replaces the row loops of index_tridist (src/dist.cpp:174-258) and index_dist
// (src/dist.cpp:560-692).
//
// A workgroup processes "units": one query row, or in the self join a pair of neighbouring rows
// (see rk_dist_kernel).  The counter row of the reference (`int intersectionArr[tid][numRef]`,
// src/dist.cpp:167) lives in LDS, two 16-bit counters per word when no count can overflow.  Per
// unit: the slices of its hashes stream from HBM into registers one per thread (the next batch is
// always in flight).  Most slices are compact (first genome + bitmask of the next 32 ids): the wave
// counts them column by column with ballots and adds each column's count with one LDS atomic; the
// few posting ranges are gathered by quads (8 postings per list and step).  The epilogue scans the
// row 16 B per lane, clears what it finds, compacts the reportable cells into an LDS list and
// evaluates the Jaccard/Mash (or containment/AafD) formula in FP64 one cell per lane; reported
// pairs are staged in LDS and flushed with one device-scope atomic per workgroup.
// The rows of a self join run in bands (plan_bands): a band's LDS rows start at its first row.
// Integer/index work: bound by vector issue and the two barriers per unit -- no MFMA.
// Developer switches (environment, read once when the context is created): RK_DIST_THREADS=256|512|768|1024,
// RK_DIST_ROWS=<units per workgroup, non-persistent>, RK_DIST_PAIR=2 (no row pairs), RK_DIST_PAIR_MINWG,
// RK_DIST_PERSIST=2 (one run per workgroup), RK_DIST_CAND_CAP, RK_DIST_STAGE_HITS, RK_DIST_XCD_ROWS, RK_DIST_BANDS=0 (one
// launch), RK_DIST_BAND_MIN_ROWS, RK_DIST_LDS_KB (plan as if a CU had less LDS: tiles and bands at test sizes).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <tuple>
#include <vector>


#include "rk_internal.h"
#include "rk_dist_common.h"
#include "rk_dist_plan.h"
#include "rk_tile_cells.h"

namespace {

// (row, col) sort key of every hit: big results are ordered on the device (a 50 M-hit dense matrix
// takes the host's std::sort more than a second)
__global__ void k_hit_keys(const rk_hit *hits, unsigned long long n, unsigned long long *keys)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = ((unsigned long long)hits[i].row << 32) | hits[i].col;
}

constexpr int kGroup = 8;                      // postings per slice walked by a quad (4 lanes x 2 postings)
constexpr uint32_t kRowsPerXcdChunk = 16;      // consecutive rows kept on one XCD (their L2 shares a clade's postings)
constexpr uint32_t kStageHitsDefault = 24;     // reported pairs staged in LDS per workgroup
constexpr uint32_t kCandCapDefault = 256;      // non-zero cells of one unit compacted in LDS (128: 3-12 % slower)

struct DistArgs {
    const uint2 *ranges;        // posting slices [x,y) of the query hashes, rows back to back
    const uint64_t *range_off;  // u64[n_query+1] offsets of each row's slices in `ranges`
    const uint64_t *size_off;   // u64[n_query+1] offsets whose differences are the sketch sizes
    const uint32_t *postings;
    const uint32_t *ref_sizes;
    const uint32_t *orig;        // internal genome id -> the caller's (null: identity); applied where a hit leaves the kernel
    const uint64_t *range_split; // pair mode: u64[n_query], a row's slices from here on are covered by its partner
    uint32_t n_query, n_ref;
    uint32_t row_first, row_step, row_block, units_per_block, n_units;
    uint32_t slot_base;          // this launch covers the unit slots slot_base .. slot_base + n_units of the shard (a band of rows)
    uint32_t col_base;           // first column of the LDS rows: a band of the self join only needs the columns behind its first row
    uint32_t tile_cols, cnt_words, pair_stride, units_per_wg, runs_per_chunk;
    int persist;                 // 1: as many workgroups as the chip holds, each walks its share of the units
    uint32_t units_per_xcd, units_per_chunk;
    uint32_t cand_cap, stage_hits;  // LDS carve-up (entries)
    uint32_t cand_flush;            // a cell list is evaluated once it holds this many entries
    int triangle, metric, kmer_size, dense_mode;
    double max_dist;
    double min_jorc;            // conservative lower bound on jaccard/containment of a reportable pair
    uint32_t min_ref_size;      // smallest non-empty reference sketch (lower bound of a containment denominator)
    rk_hit *hits;
    unsigned long long cap;
    unsigned long long *n_hits;
    int32_t *common_dense;      // optional [n_query, n_ref]
    // list mode (the fallback of rk_near_kernel): the units are the ROWS unit_list[0 .. *unit_count); the last workgroup to
    // finish resets *unit_count and *unit_done for the next launch
    const uint32_t *unit_list;
    uint32_t *unit_count, *unit_done;
    uint32_t *unit_seen_host;   // page-locked host word: the list length this launch found (hint for the next launch's grid)
};

#ifdef RK_DIST_PROFILE
// developer build only (-DRK_DIST_PROFILE, tools/dist_phase_profile.py): per-phase wave cycles
constexpr int kProfWaves = 1 << 16;
__device__ unsigned long long g_prof[kProfWaves][16];  // one row per wave, summed on the host
#define PROF_MARK(i)                                                    \
    do {                                                                \
        const long long t_now = clock64();                              \
        prof_acc[i] += t_now - prof_t;                                  \
        prof_t = t_now;                                                 \
    } while (0)
#define PROF_FENCE() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#define PROF_FLUSH()                                                                         \
    do {                                                                                     \
        const uint32_t wv = (blockIdx.x * (kDistThreads / 64) + tid / 64) % kProfWaves;      \
        if (lane == 0) {                                                                     \
            for (int i = 0; i < 12; i++) g_prof[wv][i] += (unsigned long long)prof_acc[i];   \
            g_prof[wv][12] += (unsigned long long)(clock64() - prof_t0);                     \
            g_prof[wv][13] += 1ULL;                                                          \
            g_prof[wv][14] = (unsigned long long)prof_w0;                                    \
            g_prof[wv][15] = (unsigned long long)wall_clock64();                             \
        }                                                                                    \
    } while (0)
#else
#define PROF_MARK(i)
#define PROF_FENCE()
#define PROF_FLUSH()
#endif

// U16: two 16-bit counters per LDS word.  Valid when no count can reach 65536, i.e. the
// largest query sketch has < 65536 hashes (a count never exceeds |S_q|); halves the LDS row
// and doubles the resident rows per CU.
//
// MODE
//   kFiltered: explicit queries, tiled references or dense counter output: every posting is
//              range-checked against the tile and the triangle.
//   kSelf:     the self join over the index's own "later genomes" slices, one tile: every
//              posting lands in the row unchecked.
//   kSelfPair: kSelf over PAIRS of neighbouring rows (2p, 2p+1) with one LDS row each.  A posting
//              list is sorted by genome, so the slice of row 2p for a hash starts with 2p+1
//              exactly when 2p+1 holds that hash too -- and then continues with precisely the
//              slice of row 2p+1.  Walking it once serves both rows; row 2p+1 only walks the
//              slices of hashes its partner lacks (the index stores them first, rk_index.hip
//              compact_self).  Neighbouring genomes of a sorted collection are close relatives:
//              at 10,000 genomes 41 % of all slice walks disappear.
//
// One workgroup handles units_per_wg consecutive units (a unit = a row, or a pair of rows) and
// stages the reported pairs in LDS, so the contended device-scope atomic on the hit counter is
// paid once per workgroup instead of once per reporting wave.
// Per unit: scatter all slices | barrier | scan the rows into the cell list, clearing them | barrier |
// evaluate the cells (in batches over several units from 512 threads on).  Two barriers; the evaluation
// of unit u overlaps the scattering of unit u+1 in the faster waves (cell counters alternate).  Explicit
// queries with dense output, tiled rows and the report-everything mode (-D >= 1) zero the rows per unit
// behind a third barrier.
//
// THREADS (256, 512, 768, 1024): a counter row of N columns occupies 2N (U16) or 4N bytes of the
// CU's 160 KiB, which caps the resident workgroups; bigger rows get bigger workgroups so that the
// CU keeps 16-28 waves to hide the gather latency (measured at 28,284 / 50,000 columns: 768 / 1024
// threads are 1.8x / 2.2x faster than 256).
enum { kFiltered = 0, kSelf = 1, kSelfPair = 2 };
constexpr int kBatchFromThreads = 512;  // workgroups of at least this many threads evaluate their cells in batches across units

template <bool U16, int MODE, int THREADS>
// (second launch bound: waves per SIMD the plan counts on -- 3 x 512 or 2 x 768 threads per CU are 6 per SIMD, i.e. <= 80 VGPRs)
__global__ __launch_bounds__(THREADS, (THREADS == 512 || THREADS == 768) ? 6 : 4) void rk_dist_kernel(DistArgs a)
{
    constexpr uint32_t kDistThreads = THREADS;
    constexpr bool FILTER = MODE == kFiltered;
    constexpr bool PAIR = MODE == kSelfPair;
#ifdef RK_DIST_PROFILE
    long long prof_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long prof_t = clock64();
    const long long prof_t0 = prof_t;
    const long long prof_w0 = wall_clock64();
#endif
    // one dynamic LDS region (16-byte aligned base):
    // counter row(s) | non-zero cell list | staged hits | scalars
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *cnt = lds;
    // reportable cells: one workgroup per CU (1,024 threads) collects (row, column, common, row's sketch size) over
    // SEVERAL units in two lists taking turns (BATCH); smaller workgroups keep one (cell, common) list per unit
    constexpr bool BATCH = THREADS >= kBatchFromThreads;
    uint4 *cand = reinterpret_cast<uint4 *>(lds + a.cnt_words);
    uint2 *cand2 = reinterpret_cast<uint2 *>(lds + a.cnt_words);
    rk_hit *stage = BATCH ? reinterpret_cast<rk_hit *>(cand + 2 * a.cand_cap) : reinterpret_cast<rk_hit *>(cand2 + a.cand_cap);
    uint32_t *scal = reinterpret_cast<uint32_t *>(stage + a.stage_hits);
    unsigned long long &s_base = *reinterpret_cast<unsigned long long *>(scal);
    uint32_t *s_ncand = scal + 2;   // [2] entries in the two cell lists
    uint32_t &s_cursor = scal[4];   // staged hits
    uint32_t &s_dense = scal[5];    // dense mode: reports of the unit being evaluated
    const uint32_t kCandCap = a.cand_cap, kStageHits = a.stage_hits;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63;

    // Which units this workgroup processes.
    // One run per workgroup (a.persist == 0): blockIdx.x -> a run of units_per_wg consecutive unit
    // slots.  Workgroups are dealt round-robin over the 8 XCDs, so blocks b, b+8, ... share an L2:
    // consecutive runs of one XCD are adjacent rows, while heavy (early) rows stay spread over
    // all XCDs.
    // Persistent (a.persist == 1, single tile): as many workgroups as the chip holds; each XCD owns
    // every 8th chunk of units_per_chunk units as a queue and its workgroups take the queue
    // positions s8, s8 + G/8, s8 + 2G/8, ... (G = grid size): neighbouring units still run at the
    // same time on the same XCD, and the slices of the next unit are always prefetched.  (Pulling
    // the positions with a fetch-add per unit instead was measured slower, 0.134 vs 0.122 ms: the
    // device-scope atomics cost more than the better balance at the end buys.)
    const uint32_t n_units = a.unit_list ? *a.unit_count : a.n_units;   // (list mode: known on the device only)
    // list mode: every workgroup counts itself out; the last one resets the list for the next launch
    auto leave = [&]() {
        if (a.unit_list && threadIdx.x == 0 && atomicAdd(a.unit_done, 1u) == gridDim.x * gridDim.y - 1) {
            *a.unit_count = 0;
            *a.unit_done = 0;
            if (a.unit_seen_host) __hip_atomic_store(a.unit_seen_host, n_units, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    };
    if (a.unit_list && n_units == 0) {   // the usual case of the fallback launch: nothing to do, before any LDS is touched
        leave();
        return;
    }
    const uint32_t units_per_xcd = a.unit_list ? ((n_units + 7) / 8 + a.units_per_chunk - 1) / a.units_per_chunk * a.units_per_chunk : a.units_per_xcd;
    const uint32_t xcd = blockIdx.x & 7, s8 = blockIdx.x >> 3;
    const uint32_t rpc = a.runs_per_chunk;
    const uint32_t run = ((s8 / rpc) * 8 + xcd) * rpc + s8 % rpc;
    const bool dynamic = a.persist != 0;
    const uint32_t slot0 = run * a.units_per_wg;
    if (!dynamic && slot0 >= n_units) return;
    const uint32_t col0 = a.col_base + blockIdx.y * a.tile_cols;
    const uint32_t col1 = min(a.n_ref, col0 + a.tile_cols);
    const uint32_t ncol = col1 - col0;
    if (tid == 0) {
        s_cursor = 0;
        s_ncand[0] = s_ncand[1] = 0;
    }
    // Self join, sparse report: the rows are zeroed ONCE.  A unit only increments cells behind its diagonal, its scan
    // covers exactly that stretch and clears every non-zero quad it meets, so the rows are clean again when the next unit
    // scatters: no zero pass and one barrier less per unit (the scan's barrier also fences the next scatter).
    const bool keep_clean = !FILTER && !a.dense_mode;
    if (keep_clean) {
        uint4 *z = reinterpret_cast<uint4 *>(cnt);
        for (uint32_t i = tid; i < a.cnt_words / 4; i += kDistThreads) z[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }

    const uint32_t sub = lane & 3;  // lane of the quad
    const bool tri_filter = a.triangle && !a.common_dense;
    constexpr uint32_t kPerWord = U16 ? 2 : 1;
    const uint4 *c4 = reinterpret_cast<const uint4 *>(cnt);
    const uint32_t slot_end = min(n_units, slot0 + a.units_per_wg);  // static runs
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const uint32_t row_b_cell = a.pair_stride;  // first cell of the second row of a pair

    // unit slot -> its first row.  Rows are dealt to the ranks in blocks of row_block rows
    // (block-cyclic; row_block 1 = plain interleave): this rank owns blocks row_first,
    // row_first + row_step, ...
    auto unit_row = [&](uint32_t slot) -> uint32_t {
        if (a.unit_list) return a.unit_list[slot];
        slot += a.slot_base;
        const uint32_t upb = a.units_per_block;
        const uint32_t t = upb == 1 ? slot : slot / upb;
        const uint32_t r = slot - t * upb;
        const uint64_t row = ((uint64_t)a.row_first + (uint64_t)t * a.row_step) * a.row_block + (uint64_t)r * (PAIR ? 2 : 1);
        return row < a.n_query ? (uint32_t)row : 0xFFFFFFFFu;
    };
    auto skipped = [&](uint32_t row) {
        return row == 0xFFFFFFFFu || (a.triangle && col1 <= row + 1 && !a.common_dense);
    };
    // the unit's first row, or kNone when the slot is past the end / has no work in this tile
    auto live_row = [&](uint32_t s) -> uint32_t {
        if (s == kNone || s >= n_units) return kNone;
        const uint32_t r = unit_row(s);
        return skipped(r) ? kNone : r;
    };
    // persistent mode: queue position q of XCD x -> unit slot
    auto queue_slot = [&](uint32_t x, uint32_t q) -> uint32_t {
        const uint32_t upc = a.units_per_chunk;
        return ((q / upc) * 8 + x) * upc + q % upc;
    };
    auto queue_unit = [&](uint32_t q) -> uint32_t { return q < units_per_xcd ? queue_slot(xcd, q) : kNone; };
    auto load_slice = [&](uint64_t e, uint64_t e1) -> uint2 {
        return e < e1 ? a.ranges[e] : make_uint2(0, 0);
    };
    auto bump_cell = [&](uint32_t c) {  // scatter, src/dist.cpp:199-202
        if (U16) atomicAdd(&cnt[c >> 1], (c & 1) ? 0x10000u : 1u);
        else atomicAdd(&cnt[c], 1u);
    };

    struct Gathered {  // head postings of the 4 slices a lane's quad walks in one batch
        PostingPair id[4];
        bool ok0[4], ok1[4];
    };
    // A wave walks its 64 slices in 4 steps; in step j quad q handles the slice held by lane
    // 4q+j: each lane fetches two postings (8 B), the quad the first 8 of the list.  The L1
    // looks up tags one quad per cycle, so a slice costs one lookup (two when it straddles a
    // line) and no two lookups of a step wait on the same in-flight line.
    auto gather = [&](const uint2 rg, Gathered &g) {
        auto step = [&](int j, uint32_t rx, uint32_t ry) {
            const uint32_t k = rx + 2 * sub;
            g.ok0[j] = k < ry;
            g.ok1[j] = k + 1 < ry;
            // unconditional load, postings[0..1] are always mapped
            g.id[j] = *reinterpret_cast<const PostingPair *>(a.postings + (g.ok0[j] ? k : 0));
        };
        step(0, quad_bcast<0>(rg.x), quad_bcast<0>(rg.y));
        step(1, quad_bcast<1>(rg.x), quad_bcast<1>(rg.y));
        step(2, quad_bcast<2>(rg.x), quad_bcast<2>(rg.y));
        step(3, quad_bcast<3>(rg.x), quad_bcast<3>(rg.y));
        static_assert(kGroup == 8, "a quad covers 4 lanes x 2 postings");
    };

    // evaluates one (row, j) cell; returns true when it is reported
    auto evaluate = [&](uint32_t row, int qsize, uint32_t j, int common, rk_hit &hrec) -> bool {
        const int rs = (int)a.ref_sizes[j];
        const int size0 = a.triangle ? qsize : rs;  // :215-216 / :607-608
        const int size1 = a.triangle ? rs : qsize;
        // cheap exact-safe reject before the FP64 divide + log: the distance is monotone in
        // jaccard/containment and min_jorc sits strictly below the value at the threshold
        const int denom = a.metric ? min(size0, size1) : size0 + size1 - common;
        if ((double)common < a.min_jorc * (double)denom) return false;
        const JorcDist jd = rk_distance(common, size0, size1, a.metric, a.kmer_size);
        // the caller's genome indices: a pair of the (internal) triangle is reported with its smaller index as the row,
        // like the reference's loop `for j > i` does (src/dist.cpp:207); jaccard / containment are symmetric
        uint32_t out_row = row, out_col = j;
        bool flip = false;
        if (a.orig) {
            out_row = a.orig[row];
            out_col = a.orig[j];
            flip = a.triangle && out_row > out_col;
        }
        hrec.row = flip ? out_col : out_row;
        hrec.col = flip ? out_row : out_col;
        hrec.common = common;
        hrec.size0 = flip ? size1 : size0;
        hrec.size1 = flip ? size0 : size1;
        hrec.pad_ = 0;
        hrec.jorc = jd.jorc;
        hrec.dist = jd.dist;
        return a.triangle ? (jd.dist < a.max_dist) : (jd.dist <= a.max_dist);  // :232 / :624
    };
    auto stage_hit = [&](const rk_hit &hrec) {
        const uint32_t sl = atomicAdd(&s_cursor, 1u);
        if (sl < kStageHits) stage[sl] = hrec;
        else {  // staging full: rare, pay the device-scope atomic per hit
            const unsigned long long at = atomicAdd(a.n_hits, 1ULL);
            if (at < a.cap) a.hits[at] = hrec;
        }
    };
    // Cell lists.  A row of a similarity-ordered collection yields a handful of reportable cells; evaluating them unit
    // by unit leaves one wave with ~9 busy lanes waiting on a reference-size load and an FP64 divide + log while the
    // rest of the workgroup idles at the next barrier (a third of the kernel at 50,000 genomes, one workgroup per CU).
    // The scan therefore only APPENDS (row, column, common, |row|) to the current list; once a list is half full it is
    // evaluated by the whole workgroup, one cell per lane, and the other list takes over.
    uint32_t ccur = 0;  // uniform: the list the scans append to
    auto eval_list = [&](uint32_t which, uint32_t n) {
        for (uint32_t i = tid; i < n; i += kDistThreads) {
            const uint4 e = cand[which * kCandCap + i];
            if (e.x == kNone) continue;  // a cell outside the triangle / the tile
            rk_hit hrec;
            if (evaluate(e.x, (int)e.w, e.y, (int)e.z, hrec)) stage_hit(hrec);
        }
    };

    // ---- epilogue of one unit (src/dist.cpp:207-255 / :600-682) --------------------------
    // row_a: the unit's (first) row; row_b: its pair partner or 0xFFFFFFFF
    auto epilogue = [&](uint32_t row_a, uint32_t row_b, const int qsize_a, const int qsize_b, uint32_t par) {
        uint32_t &s_total = s_dense;
        const bool has_b = PAIR && row_b != 0xFFFFFFFFu;
        if (a.common_dense) {  // never in pair mode
            int32_t *dst = a.common_dense + (size_t)row_a * a.n_ref + col0;
            for (uint32_t i = tid; i < ncol; i += kDistThreads)
                dst[i] = (int32_t)(U16 ? (cnt[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu : cnt[i]);
        }

        auto cell = [&](uint32_t c) -> uint32_t {
            return U16 ? (cnt[c >> 1] >> ((c & 1) * 16)) & 0xFFFFu : cnt[c];
        };
        // cell of the LDS region -> (row, column) and the evaluation
        auto eval_cell = [&](uint32_t c, uint32_t common) {
            const bool in_b = PAIR && c >= row_b_cell;
            const uint32_t row = in_b ? row_b : row_a;
            const uint32_t j = col0 + (in_b ? c - row_b_cell : c);
            const uint32_t jbeg = a.triangle ? max(col0, row + 1) : col0;  // :207 / :600
            rk_hit hrec;
            if (j >= jbeg && j < col1 && evaluate(row, in_b ? qsize_b : qsize_a, j, (int)common, hrec)) stage_hit(hrec);
        };
        const uint32_t jbeg_a = a.triangle ? max(col0, row_a + 1) : col0;
        uint4 *z4s = reinterpret_cast<uint4 *>(cnt);
        const uint32_t cells_end = has_b ? row_b_cell + ncol : ncol;   // cells in use
        // row-level reject while scanning: a reportable cell needs common >= min_jorc * denominator, and the
        // denominator is at least the row's sketch size (jaccard) / min(row, smallest non-empty sketch) (containment):
        // the 1-2 chance hashes shared with unrelated genomes never enter the cell list
        auto floor_common = [&](int qsize) -> uint32_t {
            const uint32_t lb = a.metric ? min((uint32_t)qsize, a.min_ref_size) : (uint32_t)qsize;
            return max(1u, (uint32_t)floor(a.min_jorc * (double)lb));
        };
        const uint32_t minc_a = floor_common(qsize_a), minc_b = has_b ? floor_common(qsize_b) : 1u;

        if (!a.dense_mode) {
            // Sparse mode: the threshold excludes distance 1.0 (== common 0), so only cells
            // that share a hash can be reported.  Scan the LDS rows 16 B per lane skipping
            // all-zero quads and compact the non-zero cells into an LDS list (one LDS atomic
            // per lane that found any), then evaluate the list one cell per lane: the FP64
            // divide + log run in parallel, not serialised on the lane that happened to own a
            // clade's adjacent columns.
            if constexpr (BATCH) {
                // both rows of a pair are scanned from the quad that holds the first row's diagonal (nothing left of it can be
                // non-zero in a triangle; in the other modes the scan starts at the row's first quad)
                const uint32_t row_quads_s = (a.pair_stride / kPerWord) / 4;
                const uint32_t q_first = ((jbeg_a - col0) / kPerWord) / 4;
                const uint32_t q_last = ((ncol + kPerWord - 1) / kPerWord + 3) / 4;   // one row's quads in use
                const uint32_t span_s = q_last - min(q_first, q_last);
                for (uint32_t i = tid; i < span_s * (has_b ? 2u : 1u); i += kDistThreads) {
                    const uint32_t which_s = has_b && i >= span_s ? 1u : 0u;
                    const uint32_t q = which_s * row_quads_s + q_first + (i - which_s * span_s);
                    const uint4 v = c4[q];
                    if ((v.x | v.y | v.z | v.w) == 0) continue;
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    const uint32_t cq = q * 4 * kPerWord;
                    const uint32_t minc = PAIR && cq >= row_b_cell ? minc_b : minc_a;  // a quad lies in one row
                    uint32_t n = 0;
#pragma unroll
                    for (int wi = 0; wi < 4; wi++) {
                        if (U16) n += ((w[wi] & 0xFFFFu) >= minc) + ((w[wi] >> 16) >= minc);
                        else n += w[wi] >= minc;
                    }
                    if (!n) {
                        if (keep_clean) z4s[q] = make_uint4(0, 0, 0, 0);
                        continue;
                    }
                    uint32_t at = atomicAdd(&s_ncand[ccur], n);
                    // a quad whose cells do not all fit stays in the row; the walk below may find only such quads, so one that
                    // fits is cleared whether or not the rows are kept clean
                    const bool fits = at + n <= kCandCap;
                    if ((FILTER || keep_clean) && fits) z4s[q] = make_uint4(0, 0, 0, 0);
                    const bool in_b = PAIR && cq >= row_b_cell;
                    const uint32_t erow = in_b ? row_b : row_a;
                    const uint32_t eq = (uint32_t)(in_b ? qsize_b : qsize_a);
                    const uint32_t jq = col0 + (in_b ? cq - row_b_cell : cq);  // column of the quad's first cell
                    const uint32_t jbeg = a.triangle ? max(col0, erow + 1) : col0;  // :207 / :600
#pragma unroll
                    for (int wi = 0; wi < 4; wi++) {
#pragma unroll
                        for (uint32_t h = 0; h < kPerWord; h++) {
                            const uint32_t common = U16 ? (w[wi] >> (16 * h)) & 0xFFFFu : w[wi];
                            if (common >= minc) {
                                const uint32_t j = jq + wi * kPerWord + h;
                                // (cells left of the diagonal / beyond the tile are never non-zero; an entry that fails
                                // the test still occupies its slot, with a row no unit has)
                                if (at < kCandCap)
                                    cand[ccur * kCandCap + at] = make_uint4(fits && j >= jbeg && j < col1 ? erow : kNone, j, common, eq);
                                at++;
                            }
                        }
                    }
                }
                PROF_MARK(2);
                __syncthreads();
                PROF_MARK(3);
                const uint32_t n_cells = s_ncand[ccur];
                if (n_cells > kCandCap) {
                    // this unit brought more cells than the list had room for: evaluate the list, walk what the scan left in
                    // the rows, and start over with the other list
                    eval_list(ccur, kCandCap);
                    for (uint32_t c = (jbeg_a - col0) + tid; c < cells_end; c += kDistThreads) {
                        const uint32_t common = cell(c);
                        if (common >= (PAIR && c >= row_b_cell ? minc_b : minc_a)) eval_cell(c, common);
                    }
                    if (tid == 0) s_ncand[ccur ^ 1] = 0;
                    ccur ^= 1;
                    __syncthreads();
                    if (keep_clean) {  // the leftovers
                        for (uint32_t i = tid; i < a.cnt_words / 4; i += kDistThreads) z4s[i] = make_uint4(0, 0, 0, 0);
                        __syncthreads();
                    }
                } else if (n_cells >= a.cand_flush) {
                    eval_list(ccur, n_cells);
                    if (tid == 0) s_ncand[ccur ^ 1] = 0;  // (its entries were evaluated at least one unit ago)
                    ccur ^= 1;
                }
            } else {
                // both rows of a pair are scanned from the quad that holds the first row's diagonal (nothing left of it can be
                // non-zero in a triangle; in the other modes the scan starts at the row's first quad)
                const uint32_t row_quads_s = (a.pair_stride / kPerWord) / 4;
                const uint32_t q_first = ((jbeg_a - col0) / kPerWord) / 4;
                const uint32_t q_last = ((ncol + kPerWord - 1) / kPerWord + 3) / 4;   // one row's quads in use
                const uint32_t span_s = q_last - min(q_first, q_last);
                for (uint32_t i = tid; i < span_s * (has_b ? 2u : 1u); i += kDistThreads) {
                    const uint32_t which_s = has_b && i >= span_s ? 1u : 0u;
                    const uint32_t q = which_s * row_quads_s + q_first + (i - which_s * span_s);
                    const uint4 v = c4[q];
                    if ((v.x | v.y | v.z | v.w) == 0) continue;
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    const uint32_t cq = q * 4 * kPerWord;
                    const uint32_t minc = PAIR && cq >= row_b_cell ? minc_b : minc_a;  // a quad lies in one row
                    uint32_t n = 0;
#pragma unroll
                    for (int wi = 0; wi < 4; wi++) {
                        if (U16) n += ((w[wi] & 0xFFFFu) >= minc) + ((w[wi] >> 16) >= minc);
                        else n += w[wi] >= minc;
                    }
                    if (!n) {
                        if (keep_clean) z4s[q] = make_uint4(0, 0, 0, 0);
                        continue;
                    }
                    uint32_t at = atomicAdd(&s_ncand[par], n);
                    // a quad whose cells do not all fit stays in the row; the walk below may find only such quads, so one that
                    // fits is cleared whether or not the rows are kept clean
                    const bool fits = at + n <= kCandCap;
                    if ((FILTER || keep_clean) && fits) z4s[q] = make_uint4(0, 0, 0, 0);
#pragma unroll
                    for (int wi = 0; wi < 4; wi++) {
#pragma unroll
                        for (uint32_t h = 0; h < kPerWord; h++) {
                            const uint32_t common = U16 ? (w[wi] >> (16 * h)) & 0xFFFFu : w[wi];
                            if (common >= minc) {
                                if (at < kCandCap) cand2[at] = make_uint2(fits ? cq + wi * kPerWord + h : kNone, common);
                                at++;
                            }
                        }
                    }
                }
                PROF_MARK(2);
                __syncthreads();
                PROF_MARK(3);
                const uint32_t n_cells = s_ncand[par];
                for (uint32_t i = tid; i < min(n_cells, kCandCap); i += kDistThreads) {
                    const uint2 cj = cand2[i];
                    if (cj.x != kNone) eval_cell(cj.x, cj.y);
                }
                if (n_cells > kCandCap) {
                    // more cells than the list holds: walk what the scan left in the rows, one cell per lane
                    for (uint32_t c = (jbeg_a - col0) + tid; c < cells_end; c += kDistThreads) {
                        const uint32_t common = cell(c);
                        if (common >= (PAIR && c >= row_b_cell ? minc_b : minc_a)) eval_cell(c, common);
                    }
                    __syncthreads();  // the rows are zeroed next
                    if (keep_clean) {
                        for (uint32_t i = tid; i < a.cnt_words / 4; i += kDistThreads) z4s[i] = make_uint4(0, 0, 0, 0);
                        __syncthreads();
                    }
                }
            }
            PROF_MARK(4);
        } else {
            // Dense mode: every cell of [jbeg, col1) can be reported.  One column per lane;
            // pass 0 counts the unit's reports, one atomic reserves their slots, pass 1
            // re-evaluates and writes them.
            for (int pass_no = 0; pass_no < 2; pass_no++) {
                uint32_t mine = 0;
                for (int which = 0; which < (has_b ? 2 : 1); which++) {
                    const uint32_t row = which ? row_b : row_a;
                    const uint32_t base = which ? row_b_cell : 0;
                    const int qsize = which ? qsize_b : qsize_a;
                    const uint32_t jbeg = a.triangle ? max(col0, row + 1) : col0;
                    for (uint32_t j = jbeg + tid; j < col1; j += kDistThreads) {
                        const int common = (int)cell(base + j - col0);
                        rk_hit hrec;
                        if (!evaluate(row, qsize, j, common, hrec)) continue;
                        if (pass_no == 0) { mine++; continue; }
                        const unsigned long long at = s_base + atomicAdd(&s_total, 1u);
                        if (at < a.cap) a.hits[at] = hrec;
                    }
                }
                if (pass_no == 0) {
                    if (mine) atomicAdd(&s_total, mine);
                    __syncthreads();
                    const uint32_t total = s_total;
                    __syncthreads();
                    if (total == 0) break;  // uniform
                    if (tid == 0) { s_base = atomicAdd(a.n_hits, (unsigned long long)total); s_total = 0; }
                    __syncthreads();
                }
            }
            __syncthreads();  // the rows are zeroed next
        }
    };

    // ---- units of this run --------------------------------------------------------------------
    // A unit's slices are one contiguous range [e0, e1) of `ranges`: the (first) row's slices and,
    // in pair mode, right behind them the partner's uncovered slices (from eb on).  `pre` always
    // holds the next batch of slices.
    struct Unit {
        uint64_t e0, eb, e1;
        uint32_t row_b;
        int qsize_a, qsize_b;  // sketch sizes of the unit's rows: fetched one unit ahead, the epilogue starts with them
    };
    auto open_unit = [&](uint32_t row_a, Unit &u) {
        u.e0 = a.range_off[row_a];
        u.eb = u.e1 = a.range_off[row_a + 1];
        u.row_b = 0xFFFFFFFFu;
        const uint64_t s0 = a.size_off[row_a], s1 = a.size_off[row_a + 1];
        u.qsize_a = (int)(s1 - s0);
        u.qsize_b = 0;
        if (PAIR && row_a + 1 < a.n_query) {
            u.row_b = row_a + 1;
            u.e1 = a.range_split[row_a + 1];  // eb == range_off[row_b]
            u.qsize_b = (int)(a.size_off[row_a + 2] - s1);
        }
    };
    // pipeline of unit slots: s_cur is processed, s_nxt is known (its slices get prefetched), the
    // one after that is being pulled
    uint32_t s_cur, s_nxt;
    const uint32_t q_step = gridDim.x >> 3;  // persistent: workgroups of this XCD
    uint32_t q_next = s8 + 2 * q_step;       // persistent: queue position of the unit after s_nxt
    if (dynamic) {
        s_cur = queue_unit(s8);
        s_nxt = queue_unit(s8 + q_step);
    } else {
        s_cur = slot0;
        s_nxt = slot0 + 1 < slot_end ? slot0 + 1 : kNone;
    }
    uint32_t row = live_row(s_cur);
    Unit cur;
    cur.e0 = cur.eb = cur.e1 = 0;
    cur.row_b = kNone;
    cur.qsize_a = cur.qsize_b = 0;
    if (row != kNone) open_unit(row, cur);
    uint2 pre = load_slice(cur.e0 + tid, cur.e1);
    uint32_t parity = 0;

    while (s_cur != kNone) {
        uint32_t s_nn = kNone;  // the unit after next
        if (dynamic) {
            s_nn = queue_unit(q_next);
            q_next += q_step;
        } else if (s_nxt != kNone && s_nxt + 1 < slot_end) s_nn = s_nxt + 1;
        // look ahead: the next unit's slice range is fetched while this unit is processed
        const uint32_t nrow = live_row(s_nxt);
        Unit nxt;
        nxt.e0 = nxt.eb = nxt.e1 = 0;
        nxt.row_b = kNone;
        nxt.qsize_a = nxt.qsize_b = 0;
        if (nrow != kNone) open_unit(nrow, nxt);

        if (!keep_clean) {
            uint4 *z4 = reinterpret_cast<uint4 *>(cnt);  // memset row (src/dist.cpp:179)
            if (!FILTER && row != kNone) {
                // self join: only columns behind the row are ever incremented and only they are read
                const uint32_t row_quads = (a.pair_stride / kPerWord) / 4;
                const uint32_t q0 = ((row + 1 - col0) / kPerWord) / 4;
                const uint32_t span = row_quads - min(q0, row_quads);
                for (uint32_t i = tid; i < span * (PAIR ? 2u : 1u); i += kDistThreads) {
                    const uint32_t which = PAIR && i >= span ? 1u : 0u;
                    z4[which * row_quads + q0 + (i - which * span)] = make_uint4(0, 0, 0, 0);
                }
            } else {
                for (uint32_t i = tid; i < a.cnt_words / 4; i += kDistThreads) z4[i] = make_uint4(0, 0, 0, 0);
            }
            if (tid == 0) {
                s_dense = 0;
                if (!BATCH) s_ncand[parity] = 0;  // per-unit cell counter, alternating so that a slow wave still reads its unit's
            }
            __syncthreads();
        }
        PROF_MARK(6);

        const uint32_t lo_id = tri_filter ? row + 1 : 0;  // ids below are not needed (j > i)
        const uint32_t row_b = cur.row_b;
        const uint64_t e0 = cur.e0, e1 = cur.e1;

        // `in_b`: the slice belongs to the partner row (scatter into its LDS row only);
        // `also_b`: a first-row slice shared with the partner (scatter into both)
        auto bump = [&](uint32_t id, bool valid, bool in_b, bool also_b) {
            const uint32_t c = id - col0;
            if (valid && (!FILTER || (c < ncol && id >= lo_id))) {
                bump_cell((PAIR && in_b ? row_b_cell : 0) + c);
                if (PAIR && also_b) bump_cell(row_b_cell + c);
            }
        };
        // adds n (a wave-level count, <= 64) to column `id` of the unit's first row or of its partner
        auto bump_n = [&](uint32_t id, uint32_t n, bool to_b) {
            const uint32_t c = id - col0;
            if (n && (!FILTER || (c < ncol && id >= lo_id))) {
                const uint32_t cellc = (PAIR && to_b ? row_b_cell : 0) + c;
                if (U16) atomicAdd(&cnt[cellc >> 1], (cellc & 1) ? n << 16 : n);
                else atomicAdd(&cnt[cellc], n);
            }
        };
        auto stream_list = [&](uint32_t sx, uint32_t sy, bool in_b, bool also_b) {  // whole wave, 2 x 64 postings in flight
            for (uint32_t k = sx + lane; k < sy; k += 128) {
                const bool ok1 = k + 64 < sy;
                const uint32_t i0 = a.postings[k], i1 = a.postings[ok1 ? k + 64 : 0];
                bump(i0, true, in_b, also_b);
                bump(i1, ok1, in_b, also_b);
            }
        };

        // A batch = up to THREADS slices of the unit, one per thread, loaded straight from HBM
        // into a register pair (no LDS staging, no barrier).
        const uint32_t nb = (uint32_t)((e1 - e0 + kDistThreads - 1) / kDistThreads);
        for (uint32_t b = 0; b < nb; b++) {
            const uint64_t at = e0 + (uint64_t)b * kDistThreads;
            const uint2 raw = pre;
            const bool held_in_b = PAIR && at + tid >= cur.eb;   // the slice this lane holds is the partner's
            if (b + 1 < nb) pre = load_slice(at + kDistThreads + tid, e1);
            else pre = load_slice(nxt.e0 + tid, nxt.e1);
            PROF_MARK(0);

            // Compact slices (rk_index.hip compact_slice: bit 31 | first genome, bitmask of the ids first .. first+31) carry
            // their posting list in the record: no posting load, no address arithmetic.  Every lane scatters its own
            // list; the wave loops as often as its longest list has bits (a handful of neighbouring strains).  The lists
            // of one row name the same few relatives, so every lane starts at a different bit (mask rotated by lane & 7):
            // an LDS atomic instruction then spreads over ~8 columns instead of queueing 64 lanes on one counter.
            const bool cpt = (raw.x >> 31) != 0;
            const uint2 rg = cpt ? make_uint2(0, 0) : make_uint2(raw.x, raw.y & 0x7FFFFFFFu);   // posting ranges for the gather path below (bit 31 of y: rk_near_kernel's near flag)
            if (__ballot(cpt)) {  // uniform
                const uint32_t first = raw.x & 0x7FFFFFFFu;
                // pair mode: a first-row slice is shared with the partner iff its first genome IS the partner, who then
                // gets every later genome of the list
                const bool c_shared = PAIR && cpt && !held_in_b && first == row_b;
                // The lists of one row name the same few relatives: scattered lane by lane, the 64 lanes of an LDS atomic
                // queue on a handful of counters (48 % of the kernel's time).  Instead the WAVE counts: every list is shifted
                // onto the 32 columns behind the unit's first row, one ballot per occupied column counts the lanes that
                // name it, lane p receives the count of column p, and ONE conflict-free atomic per row adds them.
                const uint32_t base = row + 1;
                const uint32_t rel = first - base;
                const bool fits = cpt && rel < 32u && (rel == 0 || (raw.y >> (32u - rel)) == 0);
                const uint32_t mw = fits ? raw.y << rel : 0u;
                const uint32_t ma = PAIR && held_in_b ? 0u : mw;
                const uint32_t mb = PAIR ? (held_in_b ? mw : (c_shared ? mw & ~1u : 0u)) : 0u;  // bit 0 = the partner itself
                uint32_t ca = 0, cb = 0;
                const uint32_t occupied = wave_or(ma | mb);  // uniform: the columns any list names
                count_columns<PAIR, 0>(occupied, ma, mb, ca, cb);
                bump_n(base + lane, ca, false);
                if (PAIR) bump_n(base + lane, cb, true);
                // compact lists that reach beyond those 32 columns: lane by lane, starting at rotated bits
                if (__ballot(cpt && !fits)) {
                    const uint32_t rot = lane & 7u;
                    uint32_t m = cpt && !fits ? __builtin_amdgcn_alignbit(raw.y, raw.y, rot) : 0u;  // rotate right by rot
                    while (__ballot(m != 0)) {
                        const bool v = m != 0;
                        const uint32_t k = v ? ((uint32_t)__ffs((int)m) - 1u + rot) & 31u : 0u;
                        bump(first + k, v, held_in_b, c_shared && k != 0);
                        m &= m - 1u;
                    }
                }
            }
            if (__ballot(rg.y > rg.x)) {  // uniform: some lane holds a posting range
                Gathered g;
                gather(rg, g);
                // Lists longer than 8 (2.5 % of the slices at 10,000 genomes, 1.6 per wave and
                // batch): postings 8..23 of up to four of them are requested right away, one list
                // per 16-lane row, so their latency overlaps the quad gathers instead of adding a
                // dependent round trip each; whatever is longer still is streamed by the whole wave.
                unsigned long long longs = __ballot(rg.y - rg.x > (uint32_t)kGroup);
                uint32_t lx[4] = {0, 0, 0, 0}, ly[4] = {0, 0, 0, 0};  // uniform
                int lown[4] = {0, 0, 0, 0};                           // uniform: lane holding the slice
                uint32_t qx = 0, qy = 0;                              // this lane's 16-lane row
    #pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (longs) {  // uniform
                        const int L = __ffsll((long long)longs) - 1;
                        longs &= longs - 1;
                        lown[t] = L;
                        lx[t] = __builtin_amdgcn_readlane(rg.x, L) + kGroup;
                        ly[t] = __builtin_amdgcn_readlane(rg.y, L);
                        if ((lane >> 4) == (uint32_t)t) { qx = lx[t]; qy = ly[t]; }
                    }
                }
                const uint32_t kq = qx + (lane & 15);
                const bool lokq = kq < qy;
                const uint32_t lidq = a.postings[lokq ? kq : 0];
                PROF_MARK(7);
                PROF_FENCE();
                PROF_MARK(8);
                // pair mode: a first-row slice is shared with the partner iff its first posting IS
                // the partner; the partner then gets every later posting of the list
                bool held_shared = false;  // for the slice this lane holds
                auto walk = [&](int j, bool in_b) {
                    bool shared = false;
                    if (PAIR) {
                        const uint32_t first = quad_bcast<0>(g.ok0[j] ? g.id[j].x : 0xFFFFFFFEu);  // never a row
                        shared = !in_b && first == row_b;
                        if (sub == (uint32_t)j) held_shared = shared;
                    }
                    bump(g.id[j].x, g.ok0[j], in_b, shared && sub != 0);  // the first posting is the partner itself
                    bump(g.id[j].y, g.ok1[j], in_b, shared);
                };
                const uint32_t hb = held_in_b ? 1u : 0u;
                walk(0, PAIR && quad_bcast<0>(hb) != 0);
                walk(1, PAIR && quad_bcast<1>(hb) != 0);
                walk(2, PAIR && quad_bcast<2>(hb) != 0);
                walk(3, PAIR && quad_bcast<3>(hb) != 0);
                PROF_FENCE();
                PROF_MARK(9);
                unsigned long long shared_mask = 0, in_b_mask = 0;
                if (PAIR) {
                    shared_mask = __ballot(held_shared);
                    in_b_mask = __ballot(held_in_b);
                }
                bool q_shared = false, q_in_b = false;
    #pragma unroll
                for (int t = 0; t < 4; t++)
                    if ((lane >> 4) == (uint32_t)t) {
                        q_shared = (shared_mask >> lown[t]) & 1;
                        q_in_b = (in_b_mask >> lown[t]) & 1;
                    }
                bump(lidq, lokq, q_in_b, q_shared);
    #pragma unroll
                for (int t = 0; t < 4; t++)
                    if (lx[t] + 16 < ly[t])  // uniform
                        stream_list(lx[t] + 16, ly[t], (in_b_mask >> lown[t]) & 1, (shared_mask >> lown[t]) & 1);
                while (longs) {
                    const int L = __ffsll((long long)longs) - 1;
                    longs &= longs - 1;
                    stream_list(__builtin_amdgcn_readlane(rg.x, L) + kGroup, __builtin_amdgcn_readlane(rg.y, L),
                                (in_b_mask >> L) & 1, (shared_mask >> L) & 1);
                }
            }
            PROF_FENCE();
            PROF_MARK(10);
        }
        if (nb == 0) pre = load_slice(nxt.e0 + tid, nxt.e1);  // a unit without slices still hands over the prefetch
        __syncthreads();  // all scatters of the unit done
        // (clean rows: the counter of the NEXT unit's list; every thread read it for the unit before this one ahead of the barrier)
        if (keep_clean && !BATCH && tid == 0) s_ncand[parity ^ 1] = 0;
        PROF_MARK(1);
        if (row != kNone) epilogue(row, row_b, cur.qsize_a, cur.qsize_b, parity);
        parity ^= 1;
        s_cur = s_nxt;
        s_nxt = s_nn;
        row = nrow;
        cur = nxt;
    }

    // the cells still waiting in the current list
    __syncthreads();
    if (BATCH) eval_list(ccur, min(s_ncand[ccur], kCandCap));
    // flush the staged hits of this workgroup: one device-scope atomic, coalesced 8-byte stores
    __syncthreads();
    const uint32_t n_st = min(s_cursor, kStageHits);
    PROF_MARK(11);
    PROF_FLUSH();
    leave();
    if (n_st == 0) return;
    if (tid == 0) s_base = atomicAdd(a.n_hits, (unsigned long long)n_st);
    __syncthreads();
    const unsigned long long at0 = s_base;
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(stage);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.hits);
    constexpr uint32_t kW = sizeof(rk_hit) / 8;
    for (uint32_t i = tid; i < n_st * kW; i += kDistThreads)
        if (at0 + i / kW < a.cap) dst[at0 * kW + i] = src[i];
}

#include "rk_dist_near.inc"
#include "rk_dist_tile.inc"

struct Plan {
    uint32_t n_units, tile_cols, n_tiles, cnt_words, row_words;
    uint32_t cand_cap, stage_hits, units_per_wg, threads;
    RowShard rows;  // row distribution: blocks of row_block rows dealt round-robin to row_step shards
    uint32_t units_per_block;
    uint32_t slot_base, col_base;  // a band of the self join: its first unit slot and the first column of its LDS rows
    bool persist;
    size_t lds_bytes;
    int dense_mode, mode;
    bool u16;
};

// want_self: the ranges are the index's own "later genomes" slices (self join, triangle, no dense output)
// Largest LDS footprint (bytes) with which n workgroups share a CU: the hardware hands LDS out in granules of 1,280 bytes
// (measured: a 54,240-byte workgroup comes twice per CU, a 53,216-byte one three times)
constexpr size_t kLdsGranule = 1280, kLdsPerCu = 160 * 1024;
constexpr size_t lds_for_workgroups(size_t n) { return kLdsPerCu / n / kLdsGranule * kLdsGranule; }

// n_cols: columns an LDS row must hold (the whole reference range, or what lies behind a band's first row)
int make_plan(rk_ctx *ctx, const rk_index *idx, uint32_t n_query, uint64_t max_query_size,
              const rk_dist_opts *o, bool dense_mode, bool want_self, uint32_t n_cols, Plan *p, bool allow_pair = true)
{
    if (o->kmer_size <= 0) return rk_fail(ctx, RK_ERR_ARG, "kmer_size must be positive");
    if (o->row_block < 0) return rk_fail(ctx, RK_ERR_ARG, "row_block must be >= 0");
    // counter row in LDS; tile the reference range when it does not fit
    // two 16-bit counters per word when no count can overflow: a count never exceeds the query sketch as long as
    // no genome sits twice in a posting list (sketches with repeated hashes fall back to 32-bit counters)
    p->u16 = idx->ref_sets && max_query_size < 65536;
    p->slot_base = p->col_base = 0;
    p->cand_cap = ((ctx->sw_dist_cand_cap ? ctx->sw_dist_cand_cap : kCandCapDefault) + 1) & ~1u;
    // Persistent workgroups (one tile, >= 512 threads: with 256-thread workgroups one run of two rows
    // per workgroup measured better, 0.134 vs 0.145 ms) live long, so they stage more hits before the
    // one flush at their end.  Capacity decisions below assume the bigger staging area.
    const uint64_t one_row = (uint64_t)n_cols * (p->u16 ? 2 : 4);
    const bool small_rows = one_row + (size_t)p->cand_cap * sizeof(uint2) + kStageHitsDefault * sizeof(rk_hit) + 64 <= lds_for_workgroups(7);
    p->persist = idx->n_ref && ctx->sw_dist_persist != 2;
    p->stage_hits = ctx->sw_dist_stage_hits ? ctx->sw_dist_stage_hits : 4 * kStageHitsDefault;
    // cell lists: (cell, common) per unit for workgroups below 1,024 threads; 1,024-thread workgroups (one per CU) keep two
    // lists of 16-byte entries and evaluate across units (kernel: BATCH).  Tiles are sized for the bigger layout.
    const size_t batch_extra = 2 * (size_t)p->cand_cap * sizeof(uint4) - (size_t)p->cand_cap * sizeof(uint2);
    size_t fixed = (size_t)p->cand_cap * sizeof(uint2) + p->stage_hits * sizeof(rk_hit) + 64;
    size_t lds_cu = ctx->max_lds > 160 * 1024 ? 160 * 1024 : ctx->max_lds;
    if (ctx->sw_dist_lds_kb && (size_t)ctx->sw_dist_lds_kb * 1024 < lds_cu) lds_cu = std::max<size_t>((size_t)ctx->sw_dist_lds_kb * 1024, fixed + batch_extra + 1024);
    const size_t lds_cap = lds_cu - fixed - batch_extra;
    const uint32_t max_cols = (uint32_t)(p->u16 ? lds_cap / 2 : lds_cap / 4) & ~63u;
    uint32_t tile = n_cols ? n_cols : 1;
    if (tile > max_cols) {
        const uint32_t nt = (n_cols + max_cols - 1) / max_cols;
        tile = ((n_cols + nt - 1) / nt + 63) & ~63u;
    }
    p->tile_cols = tile;
    p->n_tiles = n_cols ? (n_cols + tile - 1) / tile : 1;
    p->row_words = ((p->u16 ? (tile + 1) / 2 : tile) + 3) & ~3u;  // whole 16-byte quads

    // row distribution: blocks of row_block rows dealt round-robin to row_step shards
    p->rows = RowShard(o, n_query, kRowsPerXcdChunk);  // all rows: every block is this shard's
    p->mode = want_self && p->n_tiles == 1 ? kSelf : kFiltered;
    // pairs of neighbouring rows: blocks must hold whole pairs and two rows must fit in LDS next to
    // each other with room for at least three workgroups per CU (measured: with fewer, the lost
    // occupancy costs more than the saved walks: 14,142 columns 0.127 ms paired vs 0.113 single)
    // (pairs rest on set semantics: with a repeated hash inside a genome the "covered" test of the index build fails)
    const bool pair_ok = allow_pair && p->mode == kSelf && p->rows.row_block % 2 == 0 && idx->d_self_split && idx->ref_sets &&
                         (size_t)p->row_words * 8 + fixed + batch_extra <= lds_for_workgroups(std::max(1u, ctx->sw_dist_pair_minwg)) &&
                         ctx->sw_dist_pair != 2;
    if (pair_ok) p->mode = kSelfPair;
    const uint32_t unit_rows = p->mode == kSelfPair ? 2 : 1;
    p->units_per_block = p->rows.row_block / unit_rows;
    p->n_units = (uint32_t)std::min<uint64_t>(p->rows.my_blocks() * p->units_per_block, 0xFFFFFFF0u);
    p->cnt_words = p->row_words * unit_rows;
    if (p->mode != kSelfPair && small_rows) {  // 7 workgroups of 256 threads per CU, not persistent
        p->persist = false;
        p->stage_hits = ctx->sw_dist_stage_hits ? ctx->sw_dist_stage_hits : kStageHitsDefault;
        fixed = (size_t)p->cand_cap * sizeof(uint2) + p->stage_hits * sizeof(rk_hit) + 64;
    }
    p->lds_bytes = (size_t)p->cnt_words * 4 + fixed;
    p->persist = p->persist && p->n_tiles == 1;
    p->units_per_wg = p->persist ? 1 : (ctx->sw_dist_rows ? ctx->sw_dist_rows : (p->mode == kSelfPair ? 1u : 2u));
    // workgroup size by row size: 7 x 256 threads fit up to ~22 KiB rows; bigger rows leave room for
    // fewer workgroups, which then need more waves each
    // 7 workgroups per CU: 4 waves each; 3: 8 waves; 2: 12 waves; 1: 16 waves (measured)
    const size_t with_lists = p->lds_bytes + batch_extra;  // from 512 threads on: the two batch lists
    p->threads = p->lds_bytes <= lds_for_workgroups(7) ? 256 : (with_lists <= lds_for_workgroups(3) ? 512 : (with_lists <= lds_for_workgroups(2) ? 768 : 1024));
    if (p->mode == kSelfPair && p->threads == 256) p->threads = 512;  // two rows' slices per unit: measured better
    const uint32_t forced = ctx->sw_dist_threads;
    if (forced == 256 || forced == 512 || forced == 1024 || forced == 768) p->threads = forced;
    if (p->threads >= (uint32_t)kBatchFromThreads) p->lds_bytes += batch_extra;
    // does a pair with distance exactly 1.0 (common == 0) pass the threshold?  (decided by the caller from the EXACT
    // options: rk_dist_rows hands the kernel a threshold a few ulps wider, which must not turn -D 1.0 into a dense report)
    p->dense_mode = dense_mode ? 1 : 0;
    return RK_OK;
}

int launch_dist(rk_ctx *ctx, const rk_index *idx, const uint2 *ranges, const uint64_t *range_off,
                const uint64_t *size_off, uint32_t n_query, const rk_dist_opts *o, const Plan &p, rk_hit *hits_dev,
                uint64_t cap, unsigned long long *n_hits_dev, int32_t *dense_dev, hipStream_t stream, uint32_t *fb = nullptr)
{
    if ((!p.n_units && !fb) || !idx->n_ref) return RK_OK;
    DistArgs a;
    a.unit_list = fb ? fb + 4 : nullptr;   // fb: [0] count, [1] done, [4..] rows
    a.unit_count = fb;
    a.unit_done = fb ? fb + 1 : nullptr;
    a.unit_seen_host = fb ? idx->h_fb_seen : nullptr;
    a.ranges = ranges;
    a.range_off = range_off;
    a.range_split = p.mode == kSelfPair ? idx->d_self_split : nullptr;
    a.size_off = size_off;
    a.postings = idx->d_postings;
    a.ref_sizes = idx->d_sizes;
    a.orig = idx->relabeled ? idx->d_orig : nullptr;
    a.n_query = n_query;
    a.n_ref = idx->n_ref;
    a.row_first = p.rows.row_first;
    a.row_step = p.rows.row_step;
    a.row_block = p.rows.row_block;
    a.units_per_block = p.units_per_block;
    a.n_units = p.n_units;
    a.slot_base = p.slot_base;
    a.col_base = p.col_base;
    a.tile_cols = p.tile_cols;
    a.cnt_words = p.cnt_words;
    a.pair_stride = p.row_words * (p.u16 ? 2 : 1);
    a.triangle = o->triangle;
    a.metric = o->metric != 0;  // the reference treats any non-zero isContainment as containment
    a.kmer_size = o->kmer_size;
    a.dense_mode = p.dense_mode;
    a.max_dist = o->max_dist;
    a.min_jorc = !p.dense_mode && o->max_dist > 0.0 ? rk_min_jorc(o) : 0.0;  // (the prefilter: disabled in dense mode)
    a.min_ref_size = (uint32_t)std::min<uint64_t>(idx->min_ref_size, 0xFFFFFFFFu);
    a.hits = hits_dev;
    a.cap = cap;
    a.n_hits = n_hits_dev;
    a.common_dense = dense_dev;
    a.units_per_wg = fb ? 1 : p.units_per_wg;   // (list mode is always persistent: one unit at a time)
    const uint32_t unit_rows = p.mode == kSelfPair ? 2 : 1;
    a.runs_per_chunk = std::max<uint32_t>(1, (ctx->sw_dist_xcd_rows ? ctx->sw_dist_xcd_rows : kRowsPerXcdChunk) / (a.units_per_wg * unit_rows));
    a.cand_cap = p.cand_cap;
    a.stage_hits = p.stage_hits;
    // one workgroup per CU (rows of ~100 KB): nothing else hides the latency of evaluating a unit's handful of cells, so
    // they are collected over several units and evaluated by the whole workgroup; with several workgroups per CU the
    // others fill the gap and every unit evaluates its own cells right away
    a.cand_flush = p.cand_cap / 2;
    void (*kern)(DistArgs) = nullptr;
#define RK_PICK3(U, T)                                                                          \
    (p.mode == kSelfPair ? rk_dist_kernel<U, kSelfPair, T>                                      \
                         : (p.mode == kSelf ? rk_dist_kernel<U, kSelf, T> : rk_dist_kernel<U, kFiltered, T>))
#define RK_PICK(T) (p.u16 ? RK_PICK3(true, T) : RK_PICK3(false, T))
    if (p.threads == 256) kern = RK_PICK(256);
    else if (p.threads == 768) kern = RK_PICK(768);
    else if (p.threads == 512) kern = RK_PICK(512);
    else kern = RK_PICK(1024);
#undef RK_PICK
#undef RK_PICK3
    if (p.lds_bytes > 48 * 1024)
        RK_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)p.lds_bytes));
    const uint32_t runs = (p.n_units + a.units_per_wg - 1) / a.units_per_wg;
    const uint32_t per = 8 * a.runs_per_chunk;  // grid padded to whole XCD chunks
    uint32_t gx = (runs + per - 1) / per * per;
    a.persist = 0;
    a.units_per_chunk = a.runs_per_chunk;  // units_per_wg == 1 in persistent mode
    a.units_per_xcd = gx / 8;
    if (p.persist || fb) {
        int per_cu = rk_occupancy(ctx, (const void *)kern, (int)p.threads, p.lds_bytes);
        // (the runtime's answer has been seen to count LDS finer than the hardware allocates it: a workgroup too many per CU
        // would start only when another ends and walk its static share of the units late)
        per_cu = std::min<int>(per_cu, (int)(kLdsPerCu / ((p.lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule)));
        const uint32_t resident = ((uint32_t)std::max(1, per_cu) * (uint32_t)std::max(1, ctx->num_cu) + 7) / 8 * 8;
        if (gx > resident || fb) {  // otherwise every unit gets its own workgroup anyway (list mode: the count is on the device)
            a.persist = 1;
            // list mode: the whole chip when the previous launch over this index found rows in the list, else a token grid (the
            // list is empty as a rule; any grid walks any list)
            gx = fb ? (idx->h_fb_seen && *(volatile uint32_t *)idx->h_fb_seen == 0 ? 64u : std::min<uint32_t>(resident, 512)) : resident;
        }
    }
    hipLaunchKernelGGL(kern, dim3(gx, p.n_tiles), dim3(p.threads), p.lds_bytes, stream, a);
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}

// Bands of the self join.  Row i only counts in the columns behind it, so the rows of a shard are cut into bands whose
// LDS rows start at the band's first row: the later the band, the shorter its rows, the more workgroups share a CU --
// and where two rows fit next to each other, neighbouring rows pair up.  (50,000 genomes: rows 0-12k need the whole
// 100 KB row and one 1,024-thread workgroup per CU; from row ~39k on the kernel runs as it does for 10,000 genomes.)
// A boundary lies where the kernel variant changes (threads, mode, tiles) and at a multiple of row_step * row_block rows,
// so that a band is a contiguous range of the shard's unit slots.

int plan_bands(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, bool dense_mode, std::vector<Plan> *bands)
{
    const uint32_t n = idx->n_ref;
    Plan cur;
    int rc = make_plan(ctx, idx, n, idx->max_src_size, o, dense_mode, true, n, &cur);
    if (rc) return rc;
    bands->clear();
    const uint64_t round_rows = (uint64_t)cur.rows.row_step * cur.rows.row_block;  // one block of every shard
    const uint64_t n_rounds = ((uint64_t)n + round_rows - 1) / round_rows;
    // a band must be worth its launch (ramp-up, the tail of its last round): at least sw_dist_band_min_rows rows of THIS shard
    const uint64_t min_rounds = std::max<uint64_t>(1, ((uint64_t)ctx->sw_dist_band_min_rows + cur.rows.row_block - 1) / cur.rows.row_block);
    auto plan_at = [&](uint64_t round, Plan *q) -> int {
        const uint64_t row = round * round_rows;
        const uint32_t col_base = (uint32_t)row & ~63u;  // whole 128-byte stretches of a 16-bit row
        int prc = make_plan(ctx, idx, n, idx->max_src_size, o, dense_mode, true, n - col_base, q);
        q->col_base = col_base;
        q->slot_base = (uint32_t)(round * q->units_per_block);
        return prc;
    };
    auto differs = [&](const Plan &x, const Plan &y) { return x.threads != y.threads || x.mode != y.mode || x.n_tiles != y.n_tiles; };
    uint64_t t0 = 0;
    while (ctx->sw_dist_bands && !dense_mode) {
        const uint64_t lo = t0 + min_rounds;
        if (lo + min_rounds > n_rounds) break;
        uint64_t hi = n_rounds - min_rounds;  // lo <= hi
        Plan q;
        if ((rc = plan_at(hi, &q))) return rc;
        if (!differs(q, cur)) break;
        uint64_t a = lo;  // smallest round in [lo, hi] whose plan differs (the variant only ever changes one way)
        while (a < hi) {
            const uint64_t mid = (a + hi) / 2;
            if ((rc = plan_at(mid, &q))) return rc;
            if (differs(q, cur)) hi = mid; else a = mid + 1;
        }
        cur.n_units = (uint32_t)((a - t0) * cur.units_per_block);
        bands->push_back(cur);
        if ((rc = plan_at(a, &cur))) return rc;
        t0 = a;
    }
    cur.n_units = cur.n_units > cur.slot_base ? cur.n_units - cur.slot_base : 0;  // to the end of the shard
    bands->push_back(cur);
    return RK_OK;
}
void print_bands(const std::vector<Plan> &bands)   // RK_DIST_DEBUG: once per plan that is launched or named
{
    for (const Plan &b : bands)
        fprintf(stderr, "[rk] band: columns from %u, units %u from slot %u, kernel <%s, %d, %u>, %zu B LDS, %u tile(s)\n", b.col_base,
                b.n_units, b.slot_base, b.u16 ? "u16" : "u32", b.mode, b.threads, b.lds_bytes, b.n_tiles);
}

// The near-window self join (rk_dist_near.inc) applies when the report is sparse, the sketches are sets (compact slices
// exist, or are made on first use: plan_self answers for them) and a reportable pair needs a count the handful of chance
// hashes of a row cannot reach.
struct NearPlan {
    bool use = false, pair = false;
    int uw = 1;             // waves that share a unit
    uint32_t grid = 0;
    RowShard rows;
    uint32_t units_per_block, n_units;
    double min_jorc = 0.0;
};
NearPlan plan_near(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, bool dense_mode, double min_jorc)
{
    NearPlan np;
    if (!ctx->sw_dist_near || dense_mode || !idx->ref_sets || !idx->n_ref || o->kmer_size <= 0 || o->row_block < 0 || !(o->max_dist > 0.0))
        return np;
    np.min_jorc = min_jorc;
    // the smallest count a reportable pair of the SMALLEST sketch needs: below ~16 the chance hashes of a row reach it too
    // often and every unit would fall back (a loose -D: rk_dist_kernel alone is the better plan)
    if (floor(np.min_jorc * (double)idx->min_ref_size) < (double)ctx->sw_dist_near_min) return np;
    np.rows = RowShard(o, idx->n_ref, kRowsPerXcdChunk);  // all rows: every block is this shard's
    np.pair = np.rows.row_block % 2 == 0 && ctx->sw_dist_pair != 2;
    np.units_per_block = np.rows.row_block / (np.pair ? 2 : 1);
    np.n_units = (uint32_t)std::min<uint64_t>(np.rows.my_blocks() * np.units_per_block, 0xFFFFFFF0u);
    // waves per unit: one, unless the launch has fewer units than an eighth of the chip's wave slots -- then two share a
    // unit's steps (measured, 8,192 slots: 3,125 units 0.031 / 0.038 / 0.044 ms with 1 / 2 / 4 waves per unit, 625 units
    // 0.020 / 0.015 / 0.017 ms)
    const int per_cu = std::max(1, rk_occupancy(ctx, (const void *)rk_near_kernel<true, 1>, (int)kNearThreads, 0));
    const uint32_t wgs = (uint32_t)per_cu * (uint32_t)std::max(1, ctx->num_cu), wave_slots = wgs * (kNearThreads / 64);
    np.uw = np.n_units >= wave_slots / 8 ? 1 : 2;
    if (ctx->sw_dist_near_uw == 1 || ctx->sw_dist_near_uw == 2 || ctx->sw_dist_near_uw == 4) np.uw = ctx->sw_dist_near_uw;
    const uint32_t slots = (kNearThreads / 64) / (uint32_t)np.uw;
    np.grid = std::min<uint32_t>((np.n_units + slots - 1) / slots, wgs);
    np.use = true;
    return np;
}

// records of the self join that are posting ranges whose first genome lies within the 32-column window (near flag): the
// related lists that are wider than a compact record.  A handful per cent in a collection of small clades (a clade hash
// that also sits in an unrelated genome), most records when species are wider than the window.
__global__ void k_count_flagged(const uint2 *selfrange, uint64_t n_self, unsigned long long *acc)
{
    unsigned long long mine = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_self; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 r = selfrange[e];
        mine += !(r.x >> 31) && (r.y >> 31);
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(acc, mine);
}

// clusters wider than the window of rk_near_kernel: many such records (counted once per index, unless the build did), or a
// completed launch of rk_near_kernel that found rows in its fallback list
int near_window_too_narrow(rk_ctx *ctx, const rk_index *cidx, hipStream_t stream, bool *too_narrow)
{
    rk_index *idx = const_cast<rk_index *>(cidx);
    std::lock_guard<std::mutex> lk(idx->lazy_mu);
    if (!idx->spread_known) {
        unsigned long long flagged = 0;
        if (idx->d_selfrange && idx->n_self) {
            DevBuf<unsigned long long> acc(ctx);
            RK_HIP(ctx, acc.alloc(1));
            RK_HIP(ctx, hipMemsetAsync(acc.p, 0, 8, stream));
            const unsigned grid = (unsigned)std::min<uint64_t>((idx->n_self + 255) / 256, 4096);
            hipLaunchKernelGGL(k_count_flagged, dim3(grid), dim3(256), 0, stream, idx->d_selfrange, idx->n_self, acc.p);
            RK_HIP(ctx, hipGetLastError());
            int rc = rk_read_back(ctx, &flagged, acc.p, 8, stream);
            if (rc) return rc;
        }
        idx->spread = flagged * 8 > idx->n_self;
        idx->spread_known = 1;
    }
    *too_narrow = idx->spread || idx->fb_state == 3;
    return RK_OK;
}

// The plan of a self join: the kernel, its launch shape, and what the launch must make first.  plan_self is the ONE place that
// decides it -- launch_self launches what it says, rk_dist_kernel_name prints it -- from the index's current state; it builds
// nothing (the cached count above is its only trace).
struct SelfPlan {
    enum Kind { kTiles, kNear, kBands } kind = kBands;
    bool need_tiles = false, need_slices = false;   // a lazy product the launch must make first (and then plan again)
    double min_jorc = 0.0;
    TileShape tile;            // kTiles, once the records exist
    NearPlan near;             // kNear
    std::vector<Plan> bands;   // kBands
};

// Which kernel takes a sparse self join over set sketches -- decided by the index's SIZE AND SHAPE and the options alone, never
// by how often the index was joined before (until round 4 a resident index moved to the tile kernel at its second join: a
// benchmark loop and a user got different kernels):
//   * the index carries tile records (rk_index_build emits them from RK_DIST_TILES_MIN_GENOMES genomes on, rk_index_tiles.inc;
//     or an earlier launch built them lazily): the tile kernel -- except for small row shards of an index that ALSO has slice
//     records (a tile costs the same whatever the shard: the near-window kernel is the faster one below ~12,000 rows);
//   * no slice records (2^31 postings and more): the tile kernel, records built lazily;
//   * a sketch so small -- or a threshold so loose -- that rk_near_kernel's bound on the cells beyond its window cannot hold, or
//     clusters wider than its window (known from the build's slice records): the tile kernel, records built lazily;
//   * a completed launch of rk_near_kernel found rows in its fallback list (clusters a little wider than the window, which the
//     build cannot see): the tile kernel from then on -- the one rule that looks at an earlier launch, and only at its RESULT;
//   * RK_DIST_TILES=1 always, RK_DIST_TILES=0 never.
int plan_self(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, bool dense_mode, hipStream_t stream, SelfPlan *sp)
{
    sp->need_tiles = sp->need_slices = false;
    sp->min_jorc = o->max_dist > 0.0 ? rk_min_jorc(o) : 0.0;
    const bool can_rows = idx->d_selfrange || (!idx->slices_refused && idx->H < (1ULL << 30));   // (slice records exist or can be made: rk_index_ensure_slices)
    // (a join-only index -- rk_index_join_shard -- has tile records and no postings)
    const bool sparse_sets = !dense_mode && idx->ref_sets && ((idx->d_postings && idx->d_upos) || idx->tiles_ready) && idx->d_src_off && idx->n_ref &&
                             o->kmer_size > 0 && o->row_block >= 0 && o->max_dist > 0.0 && !idx->tiles_unusable;
    bool tiles = false;
    if (!sparse_sets || (!ctx->sw_dist_tiles && can_rows)) tiles = false;
    else if (ctx->sw_dist_tiles == 1 || !can_rows) tiles = true;
    else if (!ctx->sw_dist_near) tiles = false;   // (RK_DIST_NEAR=0 asks for the kernels with counter rows)
    else if (idx->tiles_ready) {
        const uint32_t step = o->row_step > 1 ? o->row_step : 1;
        const bool small_shard = step > 2 && idx->n_ref / step < (uint32_t)ctx->sw_dist_tiles_min_shard_rows;
        tiles = !(small_shard && idx->d_selfrange);
    } else if (floor(sp->min_jorc * (double)idx->min_ref_size) < (double)ctx->sw_dist_near_min) {
        tiles = true;   // a sketch so small that the chance hashes of a row reach its threshold: rk_near_kernel would send every row to its fallback
    } else {
        int rc = near_window_too_narrow(ctx, idx, stream, &tiles);
        if (rc) return rc;
    }
    if (tiles) {
        sp->kind = SelfPlan::kTiles;
        sp->need_tiles = !idx->tiles_ready;   // (the variant follows the launch size, which needs the tile directory)
        if (!sp->need_tiles) sp->tile = tile_launch_shape(idx, o, sp->min_jorc);
        return RK_OK;
    }
    if (!idx->d_selfrange) {   // the row kernels read slice records: an index built with tile records gets them on first use
        if (!can_rows)
            return rk_fail(ctx, RK_ERR_UNSUPPORTED, "this index has no slice records (2^31 postings or more): only sparse self joins (a threshold "
                                                    "below distance 1.0) over set sketches run on it%s", idx->tiles_unusable ? ", and its tile records "
                                                    "exceed the memory budget (lists scattered over thousands of genomes)" : "");
        sp->need_slices = true;
    }
    const bool slices_coming = sp->need_slices && idx->d_src_off && idx->wide == (idx->d_uhash64 != nullptr);   // (what rk_index_ensure_slices asks, with ref_sets)
    sp->near = slices_coming || idx->d_self_split ? plan_near(ctx, idx, o, dense_mode, sp->min_jorc) : NearPlan();
    sp->kind = sp->near.use ? SelfPlan::kNear : SelfPlan::kBands;
    return sp->near.use ? RK_OK : plan_bands(ctx, idx, o, dense_mode, &sp->bands);
}

// the fallback list of an index (allocated and zeroed once)
int ensure_fallback(rk_ctx *ctx, rk_index *idx, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(idx->lazy_mu);
    if (idx->d_fb) return RK_OK;
    DevBuf<uint32_t> fb(ctx);
    if (fb.alloc((size_t)idx->n_ref + 8) != hipSuccess) return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate the fallback list");
    RK_HIP(ctx, hipMemsetAsync(fb.p, 0, 16, stream));
    RK_HIP(ctx, hipStreamSynchronize(stream));  // once per index: a later call may come on another stream
    // (coherent: the host reads the word after hipEventQuery on an event without release-to-system semantics of its own)
    if (hipHostMalloc((void **)&idx->h_fb_seen, 64, hipHostMallocCoherent) == hipSuccess) *idx->h_fb_seen = 0xFFFFFFFFu;  // unknown: first launch at full size
    else { (void)hipGetLastError(); idx->h_fb_seen = nullptr; }
    idx->d_fb = fb.release();
    return RK_OK;
}

int launch_near(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, const NearPlan &np, rk_hit *hits_dev, uint64_t cap,
                unsigned long long *n_hits_dev, hipStream_t stream)
{
    NearArgs a;
    a.ranges = idx->d_selfrange;
    a.range_off = idx->d_self_off;
    a.range_split = idx->d_self_split;
    a.size_off = idx->d_src_off;
    a.postings = idx->d_postings;
    a.ref_sizes = idx->d_sizes;
    a.orig = idx->relabeled ? idx->d_orig : nullptr;
    a.n_ref = idx->n_ref;
    a.row_first = np.rows.row_first;
    a.row_step = np.rows.row_step;
    a.row_block = np.rows.row_block;
    a.units_per_block = np.units_per_block;
    a.n_units = np.n_units;
    a.metric = o->metric != 0;
    a.kmer_size = o->kmer_size;
    a.max_dist = o->max_dist;
    a.min_jorc = np.min_jorc;
    a.min_ref_size = (uint32_t)std::min<uint64_t>(idx->min_ref_size, 0xFFFFFFFFu);
    a.hits = hits_dev;
    a.cap = cap;
    a.n_hits = n_hits_dev;
    a.fb_count = idx->d_fb;
    a.fb_rows = idx->d_fb + 4;
    a.stage_hits = kNearStage;
    a.debug = getenv("RK_NEAR_DEBUG") ? atoi(getenv("RK_NEAR_DEBUG")) : 0;
#define RK_NEAR(P, U) hipLaunchKernelGGL((rk_near_kernel<P, U>), dim3(np.grid), dim3(kNearThreads), 0, stream, a)
    if (np.pair) { if (np.uw == 1) RK_NEAR(true, 1); else if (np.uw == 2) RK_NEAR(true, 2); else RK_NEAR(true, 4); }
    else { if (np.uw == 1) RK_NEAR(false, 1); else if (np.uw == 2) RK_NEAR(false, 2); else RK_NEAR(false, 4); }
#undef RK_NEAR
    RK_HIP(ctx, hipGetLastError());
    return RK_OK;
}

// The gate of the fallback launch (rk_internal.h, fb_state): skip it once a completed launch with these very options has shown
// the list to be empty; arm: this launch is the one whose completion will tell.
struct FbGate { unsigned char key[sizeof(rk_index::fb_key)] = {0}; bool skip = false, arm = false; };
FbGate fb_gate_begin(rk_ctx *ctx, rk_index *mut, const rk_dist_opts *o, bool dense_mode)
{
    FbGate g;
    static_assert(sizeof(rk_dist_opts) + 1 <= sizeof g.key, "key holds the options and the report mode");
    memcpy(g.key, o, sizeof(rk_dist_opts));
    g.key[sizeof(rk_dist_opts)] = dense_mode ? 1 : 0;
    if (ctx->sw_dist_fb_skip && mut->h_fb_seen) {
        std::lock_guard<std::mutex> lk(mut->lazy_mu);
        if (memcmp(g.key, mut->fb_key, sizeof g.key) != 0) {
            memcpy(mut->fb_key, g.key, sizeof g.key);
            mut->fb_state = 0;
        }
        if (mut->fb_state == 1) {
            const hipError_t qe = hipEventQuery((hipEvent_t)mut->fb_event);
            if (qe == hipSuccess) mut->fb_state = *(volatile uint32_t *)mut->h_fb_seen == 0 ? 2 : 3;
            else (void)hipGetLastError();  // hipErrorNotReady is sticky for hipGetLastError
        }
        g.skip = mut->fb_state == 2;
        if (mut->fb_state == 0) {
            if (!mut->fb_event) {
                hipEvent_t ev;
                if (hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventReleaseToSystem) == hipSuccess) mut->fb_event = ev;
                else (void)hipGetLastError();
            }
            g.arm = mut->fb_event != nullptr;
        }
    }
    return g;
}
void fb_gate_armed(rk_index *mut, const FbGate &g, hipStream_t stream)
{
    std::lock_guard<std::mutex> lk(mut->lazy_mu);
    if (mut->fb_state == 0 && memcmp(g.key, mut->fb_key, sizeof g.key) == 0 &&
        hipEventRecord((hipEvent_t)mut->fb_event, stream) == hipSuccess) mut->fb_state = 1;
}

// rk_near_kernel, then the rows whose far cells could be reportable (usually none): full counter rows, single rows, all columns
int launch_near_and_fallback(rk_ctx *ctx, rk_index *mut, const rk_dist_opts *o, bool dense_mode, const NearPlan &np, rk_hit *hits_dev,
                             uint64_t cap, unsigned long long *n_hits_dev, hipStream_t stream)
{
    int rc = ensure_fallback(ctx, mut, stream);
    if (!rc && np.n_units) rc = launch_near(ctx, mut, o, np, hits_dev, cap, n_hits_dev, stream);
    if (rc) return rc;
    const FbGate gate = fb_gate_begin(ctx, mut, o, dense_mode);
    if (gate.skip) return RK_OK;
    Plan fp;
    rk_dist_opts all = *o;
    all.row_first = 0;
    all.row_step = 1;
    rc = make_plan(ctx, mut, mut->n_ref, mut->max_src_size, &all, false, true, mut->n_ref, &fp, false);
    if (rc) return rc;
    rc = launch_dist(ctx, mut, mut->d_selfrange, mut->d_self_off, mut->d_src_off, mut->n_ref, o, fp, hits_dev, cap, n_hits_dev,
                     nullptr, stream, mut->d_fb);
    if (!rc && gate.arm) fb_gate_armed(mut, gate, stream);
    return rc;
}

int launch_self(rk_ctx *ctx, const rk_index *idx, const rk_dist_opts *o, bool dense_mode, rk_hit *hits_dev, uint64_t cap,
                unsigned long long *n_hits_dev, hipStream_t stream)
{
    rk_index *mut = const_cast<rk_index *>(idx);   // the lazy products and the state of the fallback list live in the index
    SelfPlan sp;
    int rc = plan_self(ctx, idx, o, dense_mode, stream, &sp);
    if (!rc && sp.need_tiles) {   // the plan stands once the records exist (a small row shard too: they are not built in vain) ...
        rc = rk_tiles_build(ctx, mut, stream);
        if (!rc && !idx->tiles_unusable) sp.tile = tile_launch_shape(idx, o, sp.min_jorc);
        else if (!rc) rc = plan_self(ctx, idx, o, dense_mode, stream, &sp);   // ... unless they exceed the builder's budget: one of the row kernels
    }
    if (!rc && sp.need_slices) {
        rc = rk_index_ensure_slices(ctx, mut, stream);
        if (!rc) rc = plan_self(ctx, idx, o, dense_mode, stream, &sp);
    }
    if (rc) return rc;
    if (sp.kind == SelfPlan::kTiles) return launch_tiles(ctx, idx, o, sp.min_jorc, sp.tile, hits_dev, cap, n_hits_dev, stream);
    if (sp.kind == SelfPlan::kNear) return launch_near_and_fallback(ctx, mut, o, dense_mode, sp.near, hits_dev, cap, n_hits_dev, stream);
    if (ctx->sw_dist_debug) print_bands(sp.bands);
    for (size_t b = 0; !rc && b < sp.bands.size(); b++)
        rc = launch_dist(ctx, idx, idx->d_selfrange, idx->d_self_off, idx->d_src_off, idx->n_ref, o, sp.bands[b], hits_dev, cap,
                         n_hits_dev, nullptr, stream);
    return rc;
}

// Host-side last word on the distances of the synchronous API.  The device evaluates the reference's formula in FP64 with
// its own `log`, which may differ from glibc's in the last bit: enough to print a different sixth decimal once in ~10^10
// hits, or to flip a pair that sits exactly on the threshold.  rk_dist_rows therefore lets the device report with a
// threshold a few ulps wider, recomputes jaccard / distance of every reported pair here with the host's libm -- the
// very expression of src/dist.cpp:218-231 / :239-252 -- and applies the reference's comparison to that value.
uint64_t host_exact_distances(rk_hit *h, uint64_t n, const rk_dist_opts *o)
{
    const int metric = o->metric != 0;
    auto fix = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const JorcDist jd = rk_distance(h[i].common, h[i].size0, h[i].size1, metric, o->kmer_size);
            h[i].jorc = jd.jorc;
            h[i].dist = jd.dist;
        }
    };
    const uint64_t kChunk = 8192;  // ~0.2 ms of divides and logs
    if (n < 2 * kChunk) fix(0, n);
    else {  // share the logs out (a dense report has tens of millions of pairs)
        const unsigned nt = (unsigned)std::min<uint64_t>(std::max(1u, std::thread::hardware_concurrency()), std::min<uint64_t>(16, n / kChunk));
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; t++) pool.emplace_back(fix, n * t / nt, n * (t + 1) / nt);
        for (auto &th : pool) th.join();
    }
    uint64_t w = 0;
    for (uint64_t i = 0; i < n; i++) {
        const bool keep = o->triangle ? (h[i].dist < o->max_dist) : (h[i].dist <= o->max_dist);  // :232 / :624
        if (keep) {
            if (w != i) h[w] = h[i];
            w++;
        }
    }
    return w;
}

// The n hits of a join in (row, col) order on the host (malloc): big results are ordered on the device (45,000 hits: 0.1 ms
// against 2 ms of std::sort); on any failure there the host sorts.
int download_hits_in_order(rk_ctx *ctx, const rk_hit *hits_dev, unsigned long long n, uint32_t n_query, hipStream_t stream, rk_hit **out_p)
{
    rk_hit *out = (rk_hit *)malloc((n ? n : 1) * sizeof(rk_hit));
    if (!out) return rk_fail(ctx, RK_ERR_NOMEM, "host allocation of %llu hits failed", n);
    const rk_hit *src = hits_dev;
    DevBuf<rk_hit> ordered(ctx);
    bool on_device = false;
    if (n > (ctx->single_shot ? (1ULL << 18) : 2048ULL)) {
        DevBuf<unsigned long long> keys(ctx), keys_out(ctx);
        int bits = 33;
        while (bits < 64 && (1ULL << (bits - 32)) < n_query) bits++;
        if (keys.alloc(n) == hipSuccess && keys_out.alloc(n) == hipSuccess && ordered.alloc(n) == hipSuccess) {
            hipLaunchKernelGGL(k_hit_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, hits_dev, n, keys.p);
            on_device = rk_prim_sort_hits(ctx, keys.p, keys_out.p, hits_dev, ordered.p, n, (unsigned)bits, stream) == RK_OK;
        }
        if (on_device) src = ordered.p;
        else (void)hipGetLastError();
    }
    if (n) {
        hipError_t e = hipMemcpyAsync(out, src, n * sizeof(rk_hit), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            free(out);
            return rk_fail(ctx, RK_ERR_HIP, "hit download failed: %s", hipGetErrorString(e));
        }
    }
    if (!on_device)
        std::sort(out, out + n, [](const rk_hit &x, const rk_hit &y) {
            return x.row != y.row ? x.row < y.row : x.col < y.col;
        });
    *out_p = out;
    return RK_OK;
}

}  // namespace

uint64_t rk_host_exact_distances(rk_hit *h, uint64_t n, const rk_dist_opts *o) { return host_exact_distances(h, n, o); }

#ifdef RK_DIST_PROFILE
extern "C" int rk_debug_dist_prof_raw(unsigned long long *out, unsigned long long n_waves)
{
    if (n_waves > (unsigned long long)kProfWaves) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), n_waves * 16 * 8) == hipSuccess ? 0 : -1;
}
extern "C" int rk_debug_dist_prof(unsigned long long *out16, int reset)
{
    std::vector<unsigned long long> all((size_t)kProfWaves * 16);
    if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_prof), sizeof(g_prof)) != hipSuccess) return -1;
    for (int i = 0; i < 16; i++) out16[i] = 0;
    for (size_t w = 0; w < (size_t)kProfWaves; w++)
        for (int i = 0; i < 16; i++) out16[i] += all[w * 16 + i];
    if (reset) {
        std::fill(all.begin(), all.end(), 0ULL);
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), all.data(), sizeof(g_prof)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

extern "C" {

int rk_dist_kernel_name(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries, const rk_dist_opts *opts, char *buf,
                        size_t cap)
{
    if (!ctx || !idx || !opts || !buf || !cap) return RK_ERR_ARG;
    if (queries) return rk_distq_kernel_name(ctx, idx, queries, buf, cap);
    SelfPlan sp;
    int rc = plan_self(ctx, idx, opts, rk_dense_mode(opts), ctx->stream, &sp);
    if (rc) return rc;
    if (sp.kind == SelfPlan::kTiles && sp.need_tiles)   // (the variant follows the launch size, which needs the tile directory: not built here -- this call changes nothing)
        snprintf(buf, cap, "rk_tile_kernel");
    else if (sp.kind == SelfPlan::kTiles)
        snprintf(buf, cap, "rk_tile_kernel<%du, %s>", sp.tile.threads, sp.tile.srow ? "true" : "false");
    else if (sp.kind == SelfPlan::kNear)
        snprintf(buf, cap, "rk_near_kernel<%s, %d>", sp.near.pair ? "true" : "false", sp.near.uw);
    else {
        if (ctx->sw_dist_debug) print_bands(sp.bands);
        const Plan &p = sp.bands[0];   // several bands: the variant of the first (widest rows)
        if (sp.bands.size() > 1)
            snprintf(buf, cap, "rk_dist_kernel<%s, %d, %u> [%u bands]", p.u16 ? "true" : "false", p.mode, p.threads, (unsigned)sp.bands.size());
        else
            snprintf(buf, cap, "rk_dist_kernel<%s, %d, %u>", p.u16 ? "true" : "false", p.mode, p.threads);
    }
    return RK_OK;
}

int rk_index_tile_stats(const rk_index *idx, const rk_dist_opts *opts, uint64_t out[4])
{
    if (!idx || !out) return RK_ERR_ARG;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!idx->tiles_ready) return RK_OK;
    out[0] = idx->n_tiles;
    out[2] = idx->n_tile_records;
    out[3] = idx->n_tile_slots;
    // (what a launch of the tile kernel would start, whichever kernel plan_self gives a join with these options)
    if (opts && opts->kmer_size > 0 && opts->max_dist > 0.0) out[1] = tile_launch_shape(idx, opts, rk_min_jorc(opts)).grid;
    return RK_OK;
}

int rk_dist_rows_dev(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries,
                     const rk_dist_opts *opts, rk_hit *hits_dev, uint64_t hits_cap,
                     uint64_t *n_hits_dev, void *stream)
{
    if (!ctx || !idx || !opts || !n_hits_dev || (!hits_dev && hits_cap)) return RK_ERR_ARG;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    if (queries) {  // ref-vs-query: look-up, counting and epilogue in one kernel (rk_distq.hip)
        if (opts->triangle && queries->n != idx->n_ref)
            return rk_fail(ctx, RK_ERR_ARG, "triangle mode needs the indexed sketches as queries (%u vs %u)",
                           queries->n, idx->n_ref);
        return rk_distq_launch(ctx, idx, queries, opts, rk_dense_mode(opts), hits_dev, hits_cap, (unsigned long long *)n_hits_dev,
                               nullptr, (hipStream_t)stream);
    }
    if (int rc = rk_self_join_args(ctx, idx, opts)) return rc;
    return launch_self(ctx, idx, opts, rk_dense_mode(opts), hits_dev, hits_cap, (unsigned long long *)n_hits_dev, (hipStream_t)stream);
}

int rk_dist_rows(rk_ctx *ctx, const rk_index *idx, const rk_sketches *queries,
                 const rk_dist_opts *opts, rk_hit **hits_out, uint64_t *n_hits, int32_t *common_dense)
{
    if (!ctx || !idx || !opts || !hits_out || !n_hits) return RK_ERR_ARG;
    *hits_out = nullptr;
    *n_hits = 0;
    RK_HIP(ctx, hipSetDevice(ctx->device));
    const bool self = (queries == nullptr);
    if (self)
        if (int arc = rk_self_join_args(ctx, idx, opts)) return arc;
    if (self && common_dense) return rk_fail(ctx, RK_ERR_ARG, "common_dense needs explicit query sketches");
    const uint32_t n_query = self ? idx->n_ref : queries->n;
    if (opts->triangle && n_query != idx->n_ref)
        return rk_fail(ctx, RK_ERR_ARG, "triangle mode needs the indexed sketches as queries (%u vs %u)",
                       n_query, idx->n_ref);
    int rc = RK_OK;
    // the device reports with a threshold ~64 ulps wider; host_exact_distances() decides with the host's libm.
    // Whether distance 1.0 (common == 0) is reportable -- the dense report: every cell a hit, O(n^2) records -- is decided
    // from the EXACT threshold: the default -D 1.0 of alldist (`1.0 < 1.0` is false, src/dist.cpp:232) stays sparse.
    const rk_dist_opts *exact_opts = opts;
    rk_dist_opts widened = *opts;
    if (widened.max_dist > 0.0) widened.max_dist += widened.max_dist * kBorderRel;
    opts = &widened;
    const bool dense_mode = rk_dense_mode(exact_opts);
    hipStream_t stream = ctx->stream;

    DevBuf<int32_t> dense(ctx);
    if (common_dense) {
        RK_HIP(ctx, dense.alloc((size_t)n_query * idx->n_ref));
        RK_HIP(ctx, hipMemsetAsync(dense.p, 0, (size_t)n_query * idx->n_ref * 4, stream));
    }
    DevBuf<unsigned long long> counter(ctx);
    RK_HIP(ctx, counter.alloc(1));

    // sparse mode: optimistic capacity, exact retry on overflow.  dense mode: every
    // selected (row, col) cell is a hit, so the count is known up front.
    const RowShard rows(opts, n_query, n_query);   // (all rows: one block)
    uint64_t cap = 0;
    for (uint64_t blk = rows.row_first; dense_mode && blk * rows.row_block < n_query; blk += rows.row_step)
        for (uint64_t r = blk * rows.row_block; r < std::min<uint64_t>(n_query, (blk + 1) * rows.row_block); r++)
            cap += opts->triangle ? idx->n_ref - 1 - r : idx->n_ref;
    if (!dense_mode) cap = rk_hit_capacity(rows.n_rows());
    for (int attempt = 0; attempt < 2; attempt++) {
        DevBuf<rk_hit> hits(ctx);
        if (hits.alloc(cap) != hipSuccess)
            return rk_fail(ctx, RK_ERR_NOMEM, "cannot allocate %llu hit records on the device",
                           (unsigned long long)cap);
        RK_HIP(ctx, hipMemsetAsync(counter.p, 0, 8, stream));
        if (self)
            rc = launch_self(ctx, idx, opts, dense_mode, hits.p, cap, counter.p, stream);
        else
            rc = rk_distq_launch(ctx, idx, queries, opts, dense_mode, hits.p, cap, counter.p, common_dense ? dense.p : nullptr, stream);
        if (rc) return rc;
        unsigned long long n = 0;
        rc = rk_read_back(ctx, &n, counter.p, 8, stream);
        if (rc) return rc;
        if (n > cap) {  // overflow: rerun with the exact count
            cap = n;
            continue;
        }
        rk_hit *out = nullptr;
        rc = download_hits_in_order(ctx, hits.p, n, n_query, stream, &out);
        if (rc) return rc;
        *hits_out = out;
        *n_hits = host_exact_distances(out, n, exact_opts);
        if (common_dense) {
            RK_HIP(ctx, hipMemcpyAsync(common_dense, dense.p, (size_t)n_query * idx->n_ref * 4, hipMemcpyDeviceToHost, stream));
            RK_HIP(ctx, hipStreamSynchronize(stream));
        }
        return RK_OK;
    }
    return rk_fail(ctx, RK_ERR_CAPACITY, "hit buffer overflow persisted after resize");
}

}  // extern "C"
