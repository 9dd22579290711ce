// Developer check: the host arithmetic of rk_sketch_pass.h as a stand-alone program (plain C++, no HIP, no GPU) -- prints the chunk
// length, the plan of a pass (or its refusal) with its rows, the grid, the work buffer's layout, the candidate regions of an attempt and
// the retry rule's outcome for a fixed list of cases; tests/test_sketch_pass_cpu.py compares every line with the rules as
// rk_sketch_packed_dev_ex had them inline.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -Iinclude -Irabbitkssd_amd/csrc tools/sketch_pass_check.cpp -o sketch_pass_check && ./sketch_pass_check
#include <cstdio>
#include "rk_sketch_pass.h"

typedef unsigned long long ull;
struct Range { uint64_t beg, end; };

// genomes of these lengths one after the other, each at the next multiple of 1024; *packed_bytes: the padded end of the last
static std::vector<Range> back_to_back(const std::vector<uint64_t> &bytes, uint64_t *packed_bytes)
{
    std::vector<Range> r;
    uint64_t at = 0;
    for (uint64_t b : bytes) {
        r.push_back({at, at + b});
        at = (at + b + 1023) & ~1023ULL;
    }
    *packed_bytes = at;
    return r;
}

static void plan_case(const char *name, const std::vector<Range> &gs, uint64_t packed_bytes, int drlevel, int num_cu, int img, uint64_t ov)
{
    std::vector<uint64_t> beg, end;
    for (const Range &g : gs) { beg.push_back(g.beg); end.push_back(g.end); }
    const PassPlan p = plan_pass(beg.data(), end.data(), (uint32_t)gs.size(), packed_bytes, drlevel, 4, num_cu, img, ov);
    if (p.code) { printf("plan %s : refused %d %d %u\n", name, p.code, (int)p.rule, p.bad_genome); return; }
    printf("plan %s : %u %u %u %u\n", name, p.chunk_blocks, p.n_chunks, p.grid, p.n_groups);
    for (size_t g = 0; g < p.rows.size(); g++)
        printf("row %s %zu : %llu %u %u %u\n", name, g, (ull)p.rows[g].beg, p.rows[g].nblk, p.rows[g].first_chunk, p.rows[g].reg_cap);
}

static std::vector<GenomeRow> rows_with(const std::vector<uint32_t> &caps)
{
    std::vector<GenomeRow> rows(caps.size() + 1);
    for (size_t g = 0; g < caps.size(); g++) rows[g].reg_cap = caps[g];
    return rows;
}

static void layout_case(const char *name, std::vector<GenomeRow> &rows, size_t key_bytes)
{
    const uint32_t n = (uint32_t)rows.size() - 1;
    const AttemptLayout a = layout_attempt(rows, n, key_bytes);
    printf("lay %s %zu : %llu %zu %u %u %d", name, key_bytes, (ull)a.total_cap, a.small_lds, a.n_big, a.max_reg_cap, (int)a.any_big);
    for (uint32_t g = 0; g < n; g++) printf(" | %llu %u", (ull)rows[g].reg_off, rows[g].is_big);
    printf("\n");
}

static void retry_case(const char *name, const std::vector<uint32_t> &caps, const std::vector<uint32_t> &counts, bool flag, size_t key_bytes)
{
    std::vector<GenomeRow> rows = rows_with(caps);
    const RetryOutcome r = retry_rule(rows, (uint32_t)caps.size(), counts.data(), flag);
    printf("retry %s : %d %u", name, (int)r.again, r.max_candidates);
    for (size_t g = 0; g < caps.size(); g++) printf(" %u", rows[g].reg_cap);
    printf("\n");
    layout_case(name, rows, key_bytes);   // the second attempt's regions
}

int main()
{
    const int cus[] = {1, 8, 256, 304};
    // ---- chunk length: both branches of the rule around limit = 4 * 16 * num_cu genomes, the clamps at 16 and 2^20
    for (int cu : cus) {
        const uint64_t limit = 64ull * cu;
        for (uint64_t n : {limit - 1, limit, limit + 1}) {
            const uint64_t d = n < limit ? limit - n : limit;
            for (uint64_t total : {(uint64_t)0, (uint64_t)1, 15 * d, 16 * d, 16 * d + 1, (d << 20), (d << 20) + 1})
                printf("cb %d %llu %llu 0 : %llu\n", cu, (ull)n, (ull)total, (ull)chunk_length(total, (uint32_t)n, cu, 0));
        }
    }
    for (uint64_t v : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)(1 << 20) + 1})   // RK_SKETCH_CB
        printf("cb 8 4 1000 %llu : %llu\n", (ull)v, (ull)chunk_length(1000, 4, 8, clamp_chunk_override(v)));

    // ---- rows
    uint64_t pb = 0;
    std::vector<Range> gs = back_to_back({0, 1, 1024, 1025}, &pb);
    plan_case("sizes", gs, pb, 3, 8, 1, 0);
    gs = back_to_back({3 * 1024, 4 * 1024, 3 * 1024 + 1}, &pb);   // cb, cb + 1 blocks
    plan_case("cb3", gs, pb, 3, 8, 1, 3);
    gs = back_to_back({0, 5 * 1024, 0, 0, 2 * 1024 + 1, 0}, &pb);   // empty genomes between full ones
    plan_case("gaps", gs, pb, 3, 8, 1, 2);
    gs = back_to_back({}, &pb);
    plan_case("none", gs, pb, 3, 8, 1, 0);
    gs = back_to_back({0, 0, 0}, &pb);
    plan_case("empty3", gs, pb, 3, 8, 1, 0);
    for (int dr = 1; dr <= 4; dr++) {
        char name[8];
        snprintf(name, sizeof name, "dr%d", dr);
        gs = back_to_back({1000000, 70000}, &pb);
        plan_case(name, gs, pb, dr, 304, 2, 0);
    }

    // ---- refusals
    plan_case("end_before_beg", {{0, 1024}, {2048, 2047}}, 4096, 3, 8, 1, 0);
    plan_case("beg_unaligned", {{0, 1024}, {1025, 2048}}, 4096, 3, 8, 1, 0);
    plan_case("end_beyond", {{0, 1024}, {1024, 4097}}, 4096, 3, 8, 1, 0);
    plan_case("tail_unpadded", {{0, 1024}, {2048, 2049}}, 2049, 3, 8, 1, 0);
    plan_case("tail_empty_genome", {{0, 1024}, {2048, 2048}}, 2049, 3, 8, 1, 0);
    const uint64_t max_blocks = 0x7FFFFFFFull;
    plan_case("blocks_at_31_bits", {{0, max_blocks << 10}}, max_blocks << 10, 4, 8, 1, 0);
    plan_case("blocks_beyond_31_bits", {{0, (max_blocks << 10) + 1}}, (max_blocks + 1) << 10, 4, 8, 1, 0);
    const uint64_t want_max = ((0xFFFFFFF0ull - 192) / 2) << 4;   // bytes whose region is 0xFFFFFFF0 slots at drlevel 1
    plan_case("region_at_ceiling", {{0, want_max}}, (want_max + 1023) & ~1023ULL, 1, 8, 1, 0);
    plan_case("region_beyond_ceiling", {{1024, 1024 + want_max + 16}}, (1024 + want_max + 16 + 1023) & ~1023ULL, 1, 8, 1, 0);
    plan_case("chunks_beyond_ceiling", {{0, max_blocks << 10}, {max_blocks << 10, 2 * max_blocks << 10}, {2 * max_blocks << 10, 3 * max_blocks << 10}},
              3 * max_blocks << 10, 4, 8, 1, 1);
    // (every range is checked before any region: the bad range of genome 1 is reported, not the region of genome 0)
    plan_case("range_before_region", {{0, want_max + 16}, {5, 6}}, (want_max + 16 + 1023) & ~1023ULL, 1, 8, 1, 0);

    // ---- grid and ticket groups
    for (int cu : cus)
        for (int img : {0, 1, 2})
            for (uint32_t chunks : {0u, 1u, 16u, 17u, 32u * cu, 32u * cu + 1, 496u, 512u, 640u, 9600u}) {
                uint32_t grid, groups;
                grid_rule(chunks, cu, img, &grid, &groups);
                printf("grid %d %d %u : %u %u\n", cu, img, chunks, grid, groups);
            }

    // ---- the work buffer
    for (uint32_t n : {0u, 1u, 31u, 32u}) {
        const PassLayout l = pass_layout(n);
        printf("buf %u : %zu %zu %zu %zu %zu %zu %zu\n", n, l.tail, l.off, l.gcount, l.usize, l.tickets, l.res_bytes, l.work_bytes);
    }

    // ---- candidate regions of an attempt
    std::vector<GenomeRow> rows = rows_with({16384, 16385, 192});
    layout_case("k4", rows, 4);
    rows = rows_with({8192, 8193, 100});
    layout_case("k8", rows, 8);
    rows = rows_with({16385});
    layout_case("big_only", rows, 4);
    rows = rows_with({8193, 8193});
    layout_case("big_only", rows, 8);
    rows = rows_with({});
    layout_case("none", rows, 4);
    rows = rows_with({192, 5000, 0, 1, 4097});
    layout_case("mixed", rows, 4);
    rows = rows_with({192, 5000, 0, 1, 4097});
    layout_case("mixed", rows, 8);

    // ---- retry
    retry_case("fits", {192, 1000}, {192, 7}, false, 4);
    retry_case("flag_alone", {192, 1000}, {10, 20}, true, 4);
    retry_case("one_above", {192, 1000, 300}, {10, 1001, 300}, false, 4);
    retry_case("turns_big", {192, 1000}, {10, 20000}, true, 4);
    retry_case("turns_big", {192, 1000}, {10, 8193}, true, 8);
    retry_case("none", {}, {}, false, 4);
    return 0;
}
