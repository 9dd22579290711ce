// abund_file_check.cpp -- the side-car of a counted sketch (rabbitkssd_amd/host/formats.hpp: save_abund, read_abund, abund_stats,
// write_abund_report, abund_threshold) over hand-made sets in both hash widths, empty genomes included, every refusal of the
// reader, and the layout of a counted pass (rabbitkssd_amd/csrc/rk_sketch_pass.h) against the uncounted offsets.  Plain C++ with
// its own main: built with -fsanitize=address,undefined and run by tests/test_abund_cpu.py.
//   abund_file_check <work dir>       prints "ok <n checks>", exit 1 with the failed check on stderr
#include <cstdio>
#include <string>
#include <vector>

#include "formats.hpp"
#include "rk_sketch_pass.h"

using namespace rkhost;

static int g_checks = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        g_checks++;                                                                     \
        if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// three genomes, the middle one empty; `wide` picks the hash layout (half_k - drlevel > 8)
static SketchSet hand_made(bool wide)
{
    SketchSet s;
    s.info.half_k = wide ? 11 : 8;
    s.info.half_subk = 5;
    s.info.drlevel = 2;
    s.names = {"first.fa", "nothing.fa", "reads.fq"};
    const std::vector<uint64_t> h = {3, 17, 40, 41, 0xFFFFFFFFull, 5, 6, 7, 9};
    for (uint64_t x : h) {
        if (wide) s.hashes64.push_back(x << 8 | 1);
        else s.hashes.push_back((uint32_t)x);
    }
    s.off = {0, 5, 5, 9};
    s.counts = {1, 4, 2, 2, 70, 64, 63, 1, 0xFFFFFFFFu};
    return s;
}

static std::vector<unsigned char> slurp_file(const std::string &p)
{
    std::vector<unsigned char> v;
    FILE *fp = fopen(p.c_str(), "rb");
    if (!fp) return v;
    int c;
    while ((c = fgetc(fp)) != EOF) v.push_back((unsigned char)c);
    fclose(fp);
    return v;
}
static void spit_file(const std::string &p, const std::vector<unsigned char> &v)
{
    FILE *fp = fopen(p.c_str(), "wb");
    fwrite(v.data(), 1, v.size(), fp);
    fclose(fp);
}

static void refused(const std::string &path, const SketchSet &like, const char *word)
{
    SketchSet s = like;
    std::string err;
    CHECK(!read_abund(path, s, err));
    CHECK(err.find(path) != std::string::npos);   // every refusal names the file
    CHECK(err.find(word) != std::string::npos);
    CHECK(s.counts.empty());
}

static void files(const std::string &dir, bool wide)
{
    const std::string sk = dir + (wide ? "/w.sketch" : "/n.sketch"), ab = abund_path(sk);
    SketchSet s = hand_made(wide);
    std::string err;
    CHECK(s.wide() == wide);
    CHECK(save_sketches(sk, s, err));
    CHECK(save_abund(ab, s, err));
    const std::vector<unsigned char> bytes = slurp_file(ab);
    CHECK(bytes.size() == 24 + 3 * 4 + 9 * 4);
    CHECK(memcmp(bytes.data(), "RKABUND1", 8) == 0);
    const uint32_t head[4] = {3, 0, 9, 0};   // n_genomes, reserved, total (little-endian u64)
    CHECK(memcmp(bytes.data() + 8, head, 16) == 0);
    const uint32_t sizes[3] = {5, 0, 4};
    CHECK(memcmp(bytes.data() + 24, sizes, 12) == 0);
    CHECK(memcmp(bytes.data() + 36, s.counts.data(), 36) == 0);

    SketchSet back;
    CHECK(read_sketches(sk, back, err));
    CHECK(read_abund(ab, back, err));
    CHECK(back.counts == s.counts && back.off == s.off && back.hashes == s.hashes && back.hashes64 == s.hashes64);

    // ---- the refusals
    const std::string bad = dir + "/bad.sketch.abund";
    refused(dir + "/missing.sketch.abund", back, "cannot open");
    std::vector<unsigned char> b = bytes;
    b[7] = '2';
    spit_file(bad, b);
    refused(bad, back, "magic");
    b = bytes;
    b.push_back(0);
    spit_file(bad, b);
    refused(bad, back, "length");
    b = bytes;
    b.resize(b.size() - 4);
    spit_file(bad, b);
    refused(bad, back, "length");
    b.resize(10);   // shorter than the header
    spit_file(bad, b);
    refused(bad, back, "magic");
    b = bytes;
    b[16] = 8;      // total 8 with the bytes of 9
    spit_file(bad, b);
    refused(bad, back, "length");
    b = bytes;
    b[24] = 4, b[28] = 1;   // sizes 4, 1, 4: the same total, other genomes
    spit_file(bad, b);
    refused(bad, back, "size");
    b = bytes;
    b[8] = 2;       // two genomes of (5 + 4): n_genomes disagrees; one size word more makes the length fit
    b[16] = 10;
    spit_file(bad, b);
    refused(bad, back, "number of genomes");
    b = bytes;
    memset(b.data() + 36 + 4 * 3, 0, 4);   // a count of 0
    spit_file(bad, b);
    refused(bad, back, "count of 0");
    SketchSet other = back;   // a side-car next to another .sketch: one genome fewer
    other.names.pop_back();
    other.off.pop_back();
    refused(ab, other, "number of genomes");
    SketchSet torn = s;
    torn.counts.pop_back();
    CHECK(!save_abund(bad, torn, err));

    // ---- the report: genome 0 has counts 1 4 2 2 70, genome 1 none, genome 2 has 64 63 1 2^32-1
    AbundStats a = abund_stats(back.counts.data(), 5, 64);
    CHECK(a.distinct == 5 && a.occurrences == 79 && a.largest == 70 && a.median == 2);
    CHECK(a.spectrum[1] == 1 && a.spectrum[2] == 2 && a.spectrum[4] == 1 && a.spectrum[64] == 1 && a.spectrum[3] == 0);
    a = abund_stats(back.counts.data() + 5, 0, 64);
    CHECK(a.distinct == 0 && a.occurrences == 0 && a.largest == 0 && a.median == 0);
    a = abund_stats(back.counts.data() + 5, 4, 64);   // lower median of 1 63 64 2^32-1: 63; >=64 holds two
    CHECK(a.distinct == 4 && a.occurrences == 128ull + 0xFFFFFFFFull && a.largest == 0xFFFFFFFFu && a.median == 63);
    CHECK(a.spectrum[63] == 1 && a.spectrum[64] == 2 && a.spectrum[1] == 1);
    a = abund_stats(back.counts.data(), 5, 1);        // one bin: everything is >=1
    CHECK(a.spectrum[1] == 5);
    const std::string rep = dir + "/report.txt";
    FILE *fp = fopen(rep.c_str(), "w");
    CHECK(fp != nullptr);
    write_abund_report(fp, back, 4);
    fclose(fp);
    const std::vector<unsigned char> t = slurp_file(rep);
    const std::string text(t.begin(), t.end());
    CHECK(text == "first.fa\t5\t79\t70\t2\n1\t1\n2\t2\n>=4\t2\nnothing.fa\t0\t0\t0\t0\nreads.fq\t4\t4294967423\t4294967295\t63\n1\t1\n>=4\t3\n");

    // ---- the threshold: band edges included, emptied genomes kept
    SketchSet kept;
    abund_threshold(back, 2, 64, kept);
    CHECK(kept.size() == 3 && kept.names == back.names && kept.info.half_k == back.info.half_k);
    CHECK((kept.off == std::vector<uint64_t>{0, 3, 3, 5}));
    CHECK((kept.counts == std::vector<uint32_t>{4, 2, 2, 64, 63}));
    if (wide) CHECK((kept.hashes64 == std::vector<uint64_t>{17 << 8 | 1, 40 << 8 | 1, 41 << 8 | 1, 5 << 8 | 1, 6 << 8 | 1}) && kept.hashes.empty());
    else CHECK((kept.hashes == std::vector<uint32_t>{17, 40, 41, 5, 6}) && kept.hashes64.empty());
    abund_threshold(back, 1, 0xFFFFFFFFu, kept);
    CHECK(kept.counts == back.counts && kept.off == back.off && kept.hashes == back.hashes && kept.hashes64 == back.hashes64);
    abund_threshold(back, 71, 100, kept);   // everything goes
    CHECK(kept.total() == 0 && kept.size() == 3 && (kept.off == std::vector<uint64_t>{0, 0, 0, 0}));
    const std::string sk2 = dir + "/kept.sketch";
    CHECK(save_sketches(sk2, kept, err) && save_abund(abund_path(sk2), kept, err));
    SketchSet none;
    CHECK(read_sketches(sk2, none, err) && read_abund(abund_path(sk2), none, err) && none.counts.empty() && none.size() == 3);
}

// a counted pass changes nothing of the uncounted layout: the work buffer is pass_layout's, the candidate regions layout_attempt's,
// and the counts take one slot per candidate slot in a region of their own
static void pass_offsets()
{
    for (uint32_t n : {0u, 1u, 7u, 1024u, 1500u}) {
        const PassLayout l = pass_layout(n);
        CHECK(l.tail == 0 && l.off == 16 && l.gcount == 16 + ((size_t)n + 1) * 8 && l.usize == l.gcount + (size_t)n * 4);
        CHECK(l.res_bytes == l.usize && l.tickets == ((l.usize + (size_t)n * 4 + 127) & ~(size_t)127) && l.work_bytes == l.tickets + 32 * 32 * 4);
    }
    std::vector<GenomeRow> rows(4);
    const uint32_t caps[3] = {192, 16384, 16386};
    for (int g = 0; g < 3; g++) rows[g].reg_cap = caps[g];
    const AttemptLayout a = layout_attempt(rows, 3, 4);
    CHECK(a.total_cap == 192 + 16384 + 16386 && a.n_big == 1 && a.small_lds == 65536 && a.max_reg_cap == 16386);
    CHECK(rows[0].reg_off == 0 && rows[1].reg_off == 192 && rows[2].reg_off == 192 + 16384 && rows[2].is_big && !rows[1].is_big);
    CHECK(counts_slots(a, false) == 0 && counts_slots(a, true) == a.total_cap);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: abund_file_check <work dir>\n"); return 2; }
    files(argv[1], false);
    files(argv[1], true);
    pass_offsets();
    printf("ok %d\n", g_checks);
    return 0;
}
