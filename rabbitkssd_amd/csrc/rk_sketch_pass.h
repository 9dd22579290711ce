// rk_sketch_pass.h -- the host arithmetic of one sketch pass (rk_sketch_packed_dev_ex, rk_sketch.hip): what the call refuses, the
// chunk length, the pass table, the grid and its ticket groups, the layout of the work buffer, the candidate regions of an attempt
// and the retry rule.  Nothing here launches, allocates device memory or reads the environment, and everything compiles without
// HIP (tools/sketch_pass_check.cpp, tests/test_sketch_pass_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rabbitkssd.h"

// (unit-local like the rest of rk_sketch.hip, the one unit that includes this: GenomeRow is a parameter type of its kernels)
namespace {

constexpr int kWavesPerBlock = 16;                          // waves of a scan workgroup: they share one LDS filter image
constexpr uint32_t kTicketGroups = 32, kTicketStride = 32;  // ticket counters of the scan, dwords between them
constexpr uint32_t kDedupMaxBytes = 64 * 1024;              // LDS sort capacity: 16,384 32-bit or 8,192 64-bit keys
constexpr size_t kTailBytes = 16;                           // SketchTail, the head of the work buffer
constexpr uint64_t kMaxChunkBlocks = 1u << 20;

// per-genome row of the pass table (one small upload per pass): where the genome lies in the packed buffer, which
// chunks (runs of `chunk_blocks` consecutive 1 KiB blocks, one wave each) are its own, and its candidate region
struct GenomeRow {
    uint64_t beg;          // byte offset in the packed buffer (multiple of 1024)
    uint64_t reg_off;      // first slot of the candidate region
    uint32_t nblk;         // 1 KiB blocks
    uint32_t first_chunk;  // global index of its first chunk; row[n_genomes].first_chunk = number of chunks
    uint32_t reg_cap;      // slots in the candidate region
    uint32_t is_big;       // region beyond the LDS sort capacity: device-wide sort
};
static_assert(sizeof(GenomeRow) == 32, "GenomeRow is uploaded as raw bytes");

// RK_SKETCH_CB as the pass takes it (0 is "not set" to chunk_length: a set knob is at least 1)
inline uint64_t clamp_chunk_override(uint64_t v) { return std::min<uint64_t>(kMaxChunkBlocks, std::max<uint64_t>(1, v)); }

// Chunk length: (nearly) the smallest for which there are at most two chunks per wave (2 workgroups of 16 waves per CU).
// The waves run at the same speed, so the kernel lasts ceil(chunks / waves) chunks whatever the order they are
// handed out in: 2.4 chunks per wave cost three rounds (measured: 32 blocks 0.242 ms, 38 blocks 0.211 ms on
// 128 x 5 Mb); and a chunk has a fixed cost (its genome's row, the 32 bases before it, the last partial rounds
// of its queues), so more and shorter chunks are slower too (20 blocks: 0.245 ms).
// (a genome adds at most one partial chunk: total / len + n_genomes bounds the count from above)
inline uint64_t chunk_length(uint64_t total_blocks, uint32_t n_genomes, int num_cu, uint64_t cb_override)
{
    if (cb_override) return cb_override;
    const uint64_t wave_slots = (uint64_t)num_cu * 2 * kWavesPerBlock, limit = 2 * wave_slots;
    const uint64_t cb = n_genomes < limit ? (total_blocks + (limit - n_genomes) - 1) / (limit - n_genomes) : (total_blocks + limit - 1) / limit;
    return std::min<uint64_t>(kMaxChunkBlocks, std::max<uint64_t>(16, cb));
}

// persistent scan: as many workgroups as the LDS image admits per CU (two; one with the 144 KiB image), 16 chunks a workgroup
// at least; chunks by table and ticket (chunk_range), the grid a multiple of 8 * n_groups unless there is one group
inline void grid_rule(uint32_t n_chunks, int num_cu, int img, uint32_t *grid, uint32_t *n_groups)
{
    *grid = *n_groups = 0;
    if (!n_chunks) return;
    const uint32_t want = (n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
    *grid = std::min<uint32_t>(want, (uint32_t)num_cu * (img ? 2u : 1u));
    *n_groups = std::max(1u, std::min(*grid / 16, kTicketGroups));
    if (*n_groups > 1) *grid -= *grid % (8 * *n_groups);
}

// the work buffer, byte offsets: tail | off | gcount (so far read back: res_bytes) | per-genome sketch sizes | the scan's ticket
// counters at a 128-byte boundary -- cleared with ONE fill per pass
struct PassLayout {
    size_t tail, off, gcount, usize, tickets, res_bytes, work_bytes;
};
inline PassLayout pass_layout(uint32_t n_genomes)
{
    PassLayout l;
    l.tail = 0;
    l.off = kTailBytes;
    l.gcount = l.off + ((size_t)n_genomes + 1) * 8;
    l.usize = l.res_bytes = l.gcount + (size_t)n_genomes * 4;
    l.tickets = (l.usize + (size_t)n_genomes * 4 + 127) & ~(size_t)127;
    l.work_bytes = l.tickets + kTicketGroups * kTicketStride * 4;
    return l;
}

enum PassRule { kPassOk, kPassRange, kPassPadding, kPassBlocks, kPassCeiling };   // what a refused call broke
struct PassPlan {
    std::vector<GenomeRow> rows;   // n_genomes + 1: the last one carries the number of chunks
    uint32_t n_genomes = 0, chunk_blocks = 0, n_chunks = 0, grid = 0, n_groups = 0;
    size_t key_bytes = 4;
    PassLayout at = {};
    int code = RK_OK;              // a refusal: its error code, the rule and the offending genome
    PassRule rule = kPassOk;
    uint32_t bad_genome = 0;
};
inline PassPlan plan_pass(const uint64_t *gbeg, const uint64_t *gend, uint32_t n_genomes, uint64_t packed_bytes, int drlevel, size_t key_bytes,
                          int num_cu, int img, uint64_t cb_override)
{
    PassPlan p;
    p.n_genomes = n_genomes;
    p.key_bytes = key_bytes;
    auto refuse = [&](int code, PassRule rule, uint32_t g) -> PassPlan & { p.code = code; p.rule = rule; p.bad_genome = g; return p; };
    uint64_t total_blocks = 0;
    for (uint32_t g = 0; g < n_genomes; g++) {
        if (gend[g] < gbeg[g] || (gbeg[g] & 1023) || gend[g] > packed_bytes) return refuse(RK_ERR_ARG, kPassRange, g);
        if (((gend[g] + 1023) & ~1023ULL) > packed_bytes && gend[g] > gbeg[g]) return refuse(RK_ERR_ARG, kPassPadding, g);
        if (((gend[g] - gbeg[g] + 1023) >> 10) > 0x7FFFFFFFULL) return refuse(RK_ERR_UNSUPPORTED, kPassBlocks, g);
        total_blocks += (gend[g] - gbeg[g] + 1023) >> 10;
    }
    const uint64_t cb = chunk_length(total_blocks, n_genomes, num_cu, cb_override);
    p.chunk_blocks = (uint32_t)cb;
    p.rows.resize((size_t)n_genomes + 1);
    uint64_t n_chunks64 = 0;
    for (uint32_t g = 0; g < n_genomes; g++) {
        GenomeRow &r = p.rows[g];
        r.beg = gbeg[g];
        r.nblk = (uint32_t)((gend[g] - gbeg[g] + 1023) >> 10);
        r.first_chunk = (uint32_t)n_chunks64;
        n_chunks64 += (r.nblk + cb - 1) / cb;
        // candidate region: expected survivors = windows / 16^drlevel; x2 + slack, exact retry on overflow
        const uint64_t want = 2 * ((gend[g] - gbeg[g]) >> (4 * drlevel)) + 192;
        if (want > 0xFFFFFFF0ULL || n_chunks64 > 0xFFFFFFF0ULL) return refuse(RK_ERR_UNSUPPORTED, kPassCeiling, g);
        r.reg_cap = (uint32_t)want;
    }
    p.n_chunks = (uint32_t)n_chunks64;
    p.rows[n_genomes] = GenomeRow{0, 0, 0, p.n_chunks, 0, 0};
    grid_rule(p.n_chunks, num_cu, img, &p.grid, &p.n_groups);
    p.at = pass_layout(n_genomes);
    return p;
}

// the candidate regions of one attempt: back to back in the rows' order; a region whose next power of two of keys is beyond the
// LDS sort goes to the device-wide sort, the largest of the others sizes k_dedup's LDS
struct AttemptLayout {
    uint64_t total_cap = 0;
    size_t small_lds = 0;
    uint32_t n_big = 0, max_reg_cap = 0;
    bool any_big = false;
};
inline AttemptLayout layout_attempt(std::vector<GenomeRow> &rows, uint32_t n_genomes, size_t key_bytes)
{
    AttemptLayout a;
    a.small_lds = key_bytes;
    for (uint32_t g = 0; g < n_genomes; g++) {
        rows[g].reg_off = a.total_cap;
        a.total_cap += rows[g].reg_cap;
        size_t p2 = 1;
        while (p2 < rows[g].reg_cap) p2 <<= 1;
        rows[g].is_big = p2 * key_bytes > kDedupMaxBytes;
        a.max_reg_cap = std::max(a.max_reg_cap, rows[g].reg_cap);
        if (rows[g].is_big) { a.any_big = true; a.n_big++; }
        else a.small_lds = std::max(a.small_lds, p2 * key_bytes);
    }
    return a;
}

// a counted pass (rk_sketch_*_counts) keeps one 32-bit count per slot of sorted_out, in a region of its own with the regions'
// offsets: the work buffer (PassLayout) and the candidate regions are those of the uncounted pass, which allocates no count
inline uint64_t counts_slots(const AttemptLayout &a, bool counted) { return counted ? a.total_cap : 0; }

// after the read-back: a genome that emitted more candidates than its region holds gets exactly that many on the second pass;
// `overflowed`: the device (k_dedup's flag) or the big-genome loop saw one
struct RetryOutcome {
    bool again;
    uint32_t max_candidates;
};
inline RetryOutcome retry_rule(std::vector<GenomeRow> &rows, uint32_t n_genomes, const uint32_t *gcount, bool overflowed)
{
    RetryOutcome r{overflowed, 0};
    for (uint32_t g = 0; g < n_genomes; g++) {
        r.max_candidates = std::max(r.max_candidates, gcount[g]);
        if (gcount[g] > rows[g].reg_cap) {
            r.again = true;
            rows[g].reg_cap = gcount[g];  // exact on the second pass
        }
    }
    return r;
}

}  // namespace
