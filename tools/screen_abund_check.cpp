// Developer check: the two host functions that read counts -- rk_screen_abund_lists (rk_screen.hip) and rk_mask_lists_counts (rk_mask.hip) --
// against plain restatements of their rules under the host sanitizers, as a stand-alone program.  The screen: every collection of 1 .. 3 references and a query (with a second query of every other list) over a universe of
// 5 hashes, by holder sets and sizes as tools/screen_lists_check.cpp enumerates them, with counts from {1, 2, 3} drawn per collection,
// under min_common 1 .. 2 x min_won 0 .. 1; 2,000 random cases of up to 12 references with caller-given sizes, lists with repeats in any
// order, counts with a tail up to 2^32 - 1 and every row shard of 1 .. 3; three counts of 2^32 - 1 whose sum passes 2^32; the records
// against rk_screen_lists byte for byte; the empty cases and the refusals, none of which may write.
// The restatement ranks the candidates of a row once, gives a list and its count to its member of the smallest rank, and takes sums and
// lower medians from sorted vectors; the library scans every list with the comparator and selects with std::nth_element.
// The mask: every collection of up to 2 references over 5 hashes with the 32 queries at once under every band with bounds in 0 .. 3,
// in both hash widths; 1,000 random cases per width with queries in any order, repeats and counts up to 2^32 - 1; hashes, offsets and
// statistics against rk_mask_lists byte for byte; the empty cases and the refusals.  Its restatement counts holders in a std::map.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_screen.hip rabbitkssd_amd/csrc/rk_mask.hip -x hip tools/screen_abund_check.cpp -o screen_abund_check && ./screen_abund_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>
#include "rk_internal.h"
// what rk_screen.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
int rk_read_back(rk_ctx *, void *, const void *, size_t, hipStream_t) { return -1; }
int rk_index_ensure_dir(rk_ctx *, rk_index *, hipStream_t) { return -1; }
int rk_distq_counts(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, uint32_t, uint32_t, int32_t *, hipStream_t) { return -1; }
extern "C" int rk_index_export_lists(const rk_index *, uint32_t *, uint32_t *, uint32_t *) { return -1; }
extern "C" int rk_index_export64(const rk_index *, uint32_t *, uint64_t *, uint32_t *) { return -1; }
extern "C" int rk_sketches_download(const rk_sketches *, uint32_t *, uint64_t *) { return -1; }
extern "C" int rk_sketches_download64(const rk_sketches *, uint64_t *, uint64_t *) { return -1; }
extern "C" int rk_sketches_download_counts(const rk_sketches *, uint32_t *) { return -1; }
extern "C" int rk_index_order(const rk_index *, uint32_t *) { return -1; }
extern "C" int rk_sketches_from_host(rk_ctx *, const uint32_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" int rk_sketches_from_host64(rk_ctx *, const uint64_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" int rk_sketches_from_host_counts(rk_ctx *, const void *, int, const uint32_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" void rk_sketches_free(rk_sketches *) {}
extern "C" void rk_free_host(void *p) { free(p); }

static const uint64_t kMark = 0x5A5A5A5A5A5A5A5AULL;
static const uint32_t kMark32 = 0x5A5A5A5Au;
static int failures = 0;
static unsigned long long n_calls = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

struct Case {
    std::vector<uint32_t> postings, counts, ref_sizes, query_sizes, q_counts;
    std::vector<uint64_t> q_off, q_lists, query_occ;
};

struct Cand {
    uint32_t common, size, ref;
};
static bool before(const Cand &a, const Cand &b)
{
    const uint64_t ab = (uint64_t)a.common * b.size, ba = (uint64_t)b.common * a.size;
    if (ab != ba) return ab > ba;
    if (a.size != b.size) return a.size > b.size;
    return a.ref < b.ref;
}

static void sum_median(std::vector<uint32_t> v, uint64_t *sum, uint32_t *med)
{
    *sum = 0;
    *med = 0;
    if (v.empty()) return;
    std::sort(v.begin(), v.end());
    for (const uint32_t x : v) *sum += x;
    *med = v[(v.size() - 1) / 2];
}

static void run_case(const Case &c, const rk_screen_opts &o)
{
    const uint32_t nq = (uint32_t)c.q_off.size() - 1, n_ref = (uint32_t)c.ref_sizes.size();
    if (n_ref > 32) abort();
    std::vector<uint64_t> pos(c.counts.size() + 1, 0);
    for (size_t u = 0; u < c.counts.size(); u++) pos[u + 1] = pos[u] + c.counts[u];
    const uint32_t rb = o.row_block ? o.row_block : 1, rs = o.row_step ? o.row_step : 1;
    std::vector<rk_screen_rec> want;
    std::vector<rk_screen_abund> want_ab;
    std::vector<uint64_t> want_off{0}, want_occ((size_t)3 * nq, kMark);
    for (uint32_t q = 0; q < nq; q++) {
        if (q / rb >= o.row_first && (q / rb - o.row_first) % rs == 0) {
            std::vector<uint32_t> holders, common(n_ref, 0), rank(n_ref, 0xFFFFFFFFu);
            std::vector<std::vector<uint32_t>> shared(n_ref), claimed_by(n_ref);
            uint64_t occ_matched = 0, occ_claimed = 0;
            for (uint64_t j = c.q_off[q]; j < c.q_off[q + 1]; j++) {
                const uint64_t u = c.q_lists[j];
                uint32_t bits = 0;
                for (uint64_t i = pos[u]; i < pos[u + 1]; i++) bits |= 1u << c.postings[i];
                holders.push_back(bits);
                if (bits) occ_matched += c.q_counts[j];
                for (uint32_t r = 0; r < n_ref; r++)
                    if (bits >> r & 1) {
                        common[r]++;
                        shared[r].push_back(c.q_counts[j]);
                    }
            }
            std::vector<Cand> cands;
            for (uint32_t r = 0; r < n_ref; r++)
                if (common[r] >= o.min_common) cands.push_back(Cand{common[r], c.ref_sizes[r], r});
            std::sort(cands.begin(), cands.end(), before);
            for (size_t i = 0; i < cands.size(); i++) rank[cands[i].ref] = (uint32_t)i;
            for (size_t k = 0; k < holders.size(); k++) {
                uint32_t best = 0xFFFFFFFFu;
                for (uint32_t r = 0; r < n_ref; r++)
                    if (holders[k] >> r & 1) best = std::min(best, rank[r]);
                if (best != 0xFFFFFFFFu) {
                    claimed_by[cands[best].ref].push_back(c.q_counts[c.q_off[q] + k]);
                    occ_claimed += c.q_counts[c.q_off[q] + k];
                }
            }
            uint64_t by_records = 0;
            for (uint32_t r = 0; r < n_ref; r++)
                if (common[r] >= o.min_common && claimed_by[r].size() >= o.min_won) {
                    want.push_back(rk_screen_rec{q, r, common[r], (uint32_t)claimed_by[r].size(), c.ref_sizes[r], c.query_sizes[q]});
                    rk_screen_abund ab;
                    sum_median(shared[r], &ab.occ_common, &ab.med_common);
                    sum_median(claimed_by[r], &ab.occ_won, &ab.med_won);
                    want_ab.push_back(ab);
                    CHECK(ab.occ_won <= ab.occ_common && (ab.med_won == 0) == claimed_by[r].empty());
                    by_records += ab.occ_won;
                }
            if (o.min_won == 0) CHECK(by_records == occ_claimed);
            want_occ[(size_t)3 * q] = c.query_occ[q];
            want_occ[(size_t)3 * q + 1] = occ_matched;
            want_occ[(size_t)3 * q + 2] = occ_claimed;
        }
        want_off.push_back(want.size());
    }
    std::vector<uint64_t> off((size_t)nq + 1, kMark), off2((size_t)nq + 1, kMark), occ((size_t)3 * nq, kMark);
    std::vector<uint32_t> matched(nq, kMark32), n_cand(nq, kMark32), claimed(nq, kMark32), matched2(nq, kMark32), n_cand2(nq, kMark32), claimed2(nq, kMark32);
    rk_screen_rec *recs = (rk_screen_rec *)(uintptr_t)kMark, *recs2 = nullptr;
    rk_screen_abund *ab = (rk_screen_abund *)(uintptr_t)kMark;
    uint64_t n = kMark, n2 = kMark;
    n_calls++;
    const uint32_t *P = c.postings.empty() ? nullptr : c.postings.data(), *C = c.counts.empty() ? nullptr : c.counts.data();
    const uint64_t *QL = c.q_lists.empty() ? nullptr : c.q_lists.data();
    const int rc = rk_screen_abund_lists(P, C, c.counts.size(), c.q_off.data(), QL, c.q_counts.empty() ? nullptr : c.q_counts.data(), nq, n_ref,
                                         n_ref ? c.ref_sizes.data() : nullptr, nq ? c.query_sizes.data() : nullptr, nq ? c.query_occ.data() : nullptr, &o, off.data(), &recs,
                                         &ab, &n, nq ? matched.data() : nullptr, nq ? n_cand.data() : nullptr, nq ? claimed.data() : nullptr, nq ? occ.data() : nullptr);
    CHECK(rc == RK_OK);
    if (rc != RK_OK) return;
    CHECK(off == want_off && n == want.size() && (recs == nullptr) == want.empty() && (ab == nullptr) == want.empty());
    CHECK(want.empty() || !memcmp(recs, want.data(), want.size() * sizeof(rk_screen_rec)));
    for (size_t i = 0; i < want.size() && ab; i++)
        CHECK(ab[i].occ_common == want_ab[i].occ_common && ab[i].occ_won == want_ab[i].occ_won && ab[i].med_common == want_ab[i].med_common &&
              ab[i].med_won == want_ab[i].med_won);
    CHECK(occ == want_occ);   // (the entries of unselected rows keep their mark)
    // the records, byte for byte those of rk_screen_lists
    CHECK(rk_screen_lists(P, C, c.counts.size(), c.q_off.data(), QL, nq, n_ref, n_ref ? c.ref_sizes.data() : nullptr, nq ? c.query_sizes.data() : nullptr, &o, off2.data(),
                          &recs2, &n2, nq ? matched2.data() : nullptr, nq ? n_cand2.data() : nullptr, nq ? claimed2.data() : nullptr) == RK_OK);
    CHECK(off2 == off && n2 == n && matched2 == matched && n_cand2 == n_cand && claimed2 == claimed && (!n || !memcmp(recs, recs2, n * sizeof(rk_screen_rec))));
    rk_free_host(recs);
    rk_free_host(recs2);
    rk_free_host(ab);
}

struct Together {   // several small collections in one call per option, as tools/screen_lists_check.cpp
    Case all;
    uint32_t n = 0;
    void add(const Case &c)
    {
        const uint32_t r0 = (uint32_t)all.ref_sizes.size();
        const uint64_t u0 = all.counts.size(), j0 = all.q_lists.size();
        if (all.q_off.empty()) all.q_off.push_back(0);
        for (const uint32_t p : c.postings) all.postings.push_back(p + r0);
        all.counts.insert(all.counts.end(), c.counts.begin(), c.counts.end());
        all.ref_sizes.insert(all.ref_sizes.end(), c.ref_sizes.begin(), c.ref_sizes.end());
        all.query_sizes.insert(all.query_sizes.end(), c.query_sizes.begin(), c.query_sizes.end());
        all.query_occ.insert(all.query_occ.end(), c.query_occ.begin(), c.query_occ.end());
        all.q_counts.insert(all.q_counts.end(), c.q_counts.begin(), c.q_counts.end());
        for (const uint64_t u : c.q_lists) all.q_lists.push_back(u + u0);
        for (size_t q = 1; q < c.q_off.size(); q++) all.q_off.push_back(c.q_off[q] + j0);
        n++;
    }
    void run()
    {
        if (!n) return;
        for (uint32_t mc = 1; mc <= 2; mc++)
            for (uint32_t mw = 0; mw <= 1; mw++) run_case(all, rk_screen_opts{mc, mw, 0, 0, 0});
        all = Case();
        n = 0;
    }
};

static unsigned long long small_cases(uint32_t n_ref, std::mt19937_64 &rng)
{
    unsigned long long seen = 0;
    const uint32_t H = 5, n_masks = 1u << n_ref;
    Together together;
    for (uint32_t k = 0; k <= H; k++) {
        std::vector<uint32_t> holders(k, 0);   // non-descending masks: a multiset
        for (bool more = true; more;) {
            std::vector<uint32_t> outside(n_ref, 0);
            for (bool more_sizes = true; more_sizes;) {
                Case c;
                c.ref_sizes.assign(n_ref, 0);
                for (uint32_t h = 0; h < k; h++) {
                    uint32_t len = 0;
                    for (uint32_t r = 0; r < n_ref; r++)
                        if (holders[h] >> r & 1) {
                            c.postings.push_back(r);
                            c.ref_sizes[r]++;
                            len++;
                        }
                    c.counts.push_back(len);
                }
                for (uint32_t r = 0; r < n_ref; r++) c.ref_sizes[r] += outside[r];
                c.q_off = {0, k, k + (k + 1) / 2};
                for (uint32_t h = 0; h < k; h++) c.q_lists.push_back(h);
                for (uint32_t h = 0; h < k; h += 2) c.q_lists.push_back(h);   // the second query: every other hash (and one nobody indexes)
                c.query_sizes = {k, (k + 1) / 2 + 1};
                c.query_occ = {0, 1 + rng() % 3};
                for (size_t j = 0; j < c.q_lists.size(); j++) {
                    c.q_counts.push_back(1 + (uint32_t)(rng() % 3));
                    c.query_occ[j < k ? 0 : 1] += c.q_counts.back();
                }
                together.add(c);
                if (together.n == 32 / n_ref) together.run();
                seen++;
                more_sizes = false;
                for (uint32_t r = 0; r < n_ref && !more_sizes; r++) {
                    if (outside[r] < H - k) {
                        outside[r]++;
                        more_sizes = true;
                    } else {
                        outside[r] = 0;
                    }
                }
            }
            int i = (int)k - 1;
            while (i >= 0 && holders[(size_t)i] == n_masks - 1) i--;
            if (i < 0) {
                more = false;
            } else {
                const uint32_t v = holders[(size_t)i] + 1;
                for (uint32_t j = (uint32_t)i; j < k; j++) holders[j] = v;
            }
        }
    }
    together.run();
    return seen;
}

static void random_cases(std::mt19937_64 &rng, int n_cases)
{
    for (int t = 0; t < n_cases; t++) {
        Case c;
        const uint32_t N = (uint32_t)(rng() % 13);
        const int n_lists = N ? (int)(rng() % 26) : 0;
        std::vector<uint32_t> held(N, 0);
        for (int u = 0; u < n_lists; u++) {
            c.counts.push_back((uint32_t)(rng() % 7));
            std::set<uint32_t> once;
            for (uint32_t j = 0; j < c.counts.back(); j++) {
                c.postings.push_back((uint32_t)(rng() % N));   // any order, repeats
                once.insert(c.postings.back());
            }
            for (const uint32_t r : once) held[r]++;
        }
        for (uint32_t r = 0; r < N; r++) c.ref_sizes.push_back(held[r] + (uint32_t)(rng() % 4) * (uint32_t)(rng() % 3));
        c.q_off.push_back(0);
        for (int i = 0, n = (int)(rng() % 7); i < n; i++) {
            std::set<uint64_t> mine;
            for (int j = 0, m = n_lists ? (int)(rng() % 20) * (int)(rng() % 3 != 0) : 0; j < m; j++) mine.insert(rng() % n_lists);
            c.q_lists.insert(c.q_lists.end(), mine.begin(), mine.end());
            c.q_off.push_back(c.q_lists.size());
            c.query_sizes.push_back((uint32_t)mine.size() + (uint32_t)(rng() % 5));
            uint64_t occ = rng() % 9;
            for (size_t j = 0; j < mine.size(); j++) {
                const uint64_t kind = rng() % 16;   // mostly small, ties common; a tail up to the largest count
                c.q_counts.push_back(kind == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 3) : kind == 1 ? (uint32_t)(rng() >> 33) + 1 : 1 + (uint32_t)(rng() % 4));
                occ += c.q_counts.back();
            }
            c.query_occ.push_back(occ);
        }
        const uint32_t mc = (uint32_t)(rng() % 3) + 1, mw = (uint32_t)(rng() % 3);
        run_case(c, rk_screen_opts{mc, mw, 0, 0, 0});
        const uint32_t step = (uint32_t)(rng() % 3) + 1;
        for (uint32_t first = 0; first < step; first++) run_case(c, rk_screen_opts{mc, mw, first, step, (uint32_t)(rng() % 3)});
    }
}

// three lists held by one reference, three counts of 2^32 - 1: the sums pass 2^32, the medians stay
static void beyond_32_bits()
{
    Case c;
    c.postings = {0, 0, 0, 1};
    c.counts = {1, 1, 2};
    c.ref_sizes = {3, 1};
    c.q_off = {0, 3};
    c.q_lists = {0, 1, 2};
    c.q_counts = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    c.query_sizes = {3};
    c.query_occ = {3ULL * 0xFFFFFFFFULL};
    run_case(c, rk_screen_opts{1, 0, 0, 0, 0});
    uint64_t off[2], n = 0, occ[3];
    uint32_t matched, n_cand, claimed;
    rk_screen_rec *recs = nullptr;
    rk_screen_abund *ab = nullptr;
    const rk_screen_opts o{1, 0, 0, 0, 0};
    CHECK(rk_screen_abund_lists(c.postings.data(), c.counts.data(), 3, c.q_off.data(), c.q_lists.data(), c.q_counts.data(), 1, 2, c.ref_sizes.data(), c.query_sizes.data(),
                                c.query_occ.data(), &o, off, &recs, &ab, &n, &matched, &n_cand, &claimed, occ) == RK_OK);
    CHECK(n == 2 && ab && ab[0].occ_common == 3ULL * 0xFFFFFFFFULL && ab[0].occ_won == 3ULL * 0xFFFFFFFFULL && ab[0].med_common == 0xFFFFFFFFu &&
          ab[0].med_won == 0xFFFFFFFFu && ab[1].occ_common == 0xFFFFFFFFULL && ab[1].occ_won == 0 && ab[1].med_won == 0 && occ[1] == 3ULL * 0xFFFFFFFFULL);
    rk_free_host(recs);
    rk_free_host(ab);
}

static void refusals()
{
    const uint32_t postings[3] = {0, 1, 1}, counts[2] = {2, 1}, sizes[2] = {1, 2}, qsizes[2] = {2, 1}, small[2] = {1, 1}, qc[3] = {2, 1, 5}, zero_count[3] = {2, 0, 5};
    const uint64_t q_off[3] = {0, 2, 3}, ql[3] = {0, 1, 1}, qocc[2] = {4, 5}, far[3] = {0, 2, 1};
    const rk_screen_opts o{1, 0, 0, 0, 0}, zero{0, 0, 0, 0, 0};
    uint64_t off[3] = {kMark, kMark, kMark}, n = kMark, occ[6] = {kMark, kMark, kMark, kMark, kMark, kMark};
    uint32_t matched[2] = {kMark32, kMark32}, n_cand[2] = {kMark32, kMark32}, claimed[2] = {kMark32, kMark32};
    rk_screen_rec *recs = (rk_screen_rec *)(uintptr_t)kMark;
    rk_screen_abund *ab = (rk_screen_abund *)(uintptr_t)kMark;
#define LISTS(P, QL, QC, S, QOCC, O, R, AB, OCC) \
    rk_screen_abund_lists(P, counts, 2, q_off, QL, QC, 2, 2, S, qsizes, QOCC, O, off, R, AB, &n, matched, n_cand, claimed, OCC)
    CHECK(LISTS(postings, ql, nullptr, sizes, qocc, &o, &recs, &ab, occ) == RK_ERR_ARG);      // the new null arrays
    CHECK(LISTS(postings, ql, qc, sizes, nullptr, &o, &recs, &ab, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, qc, sizes, qocc, &o, &recs, nullptr, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, qc, sizes, qocc, &o, &recs, &ab, nullptr) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, zero_count, sizes, qocc, &o, &recs, &ab, occ) == RK_ERR_ARG);   // a count of 0
    CHECK(LISTS(nullptr, ql, qc, sizes, qocc, &o, &recs, &ab, occ) == RK_ERR_ARG);            // and what rk_screen_lists refuses
    CHECK(LISTS(postings, nullptr, qc, sizes, qocc, &o, &recs, &ab, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, far, qc, sizes, qocc, &o, &recs, &ab, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, qc, small, qocc, &o, &recs, &ab, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, qc, sizes, qocc, &zero, &recs, &ab, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, qc, sizes, qocc, nullptr, &recs, &ab, occ) == RK_ERR_ARG);
    CHECK(LISTS(postings, ql, qc, sizes, qocc, &o, nullptr, &ab, occ) == RK_ERR_ARG);
    CHECK(recs == (rk_screen_rec *)(uintptr_t)kMark && ab == (rk_screen_abund *)(uintptr_t)kMark && n == kMark && off[0] == kMark && off[2] == kMark &&
          matched[0] == kMark32 && n_cand[1] == kMark32 && claimed[0] == kMark32 && occ[0] == kMark && occ[5] == kMark);
    // the good call: list 0 (count 2) is held by 0 and 1, list 1 (counts 1 and 5) by 1 alone; 1/1 beats 2/2 by the ... larger size: 1 wins
    CHECK(LISTS(postings, ql, qc, sizes, qocc, &o, &recs, &ab, occ) == RK_OK);
    CHECK(n == 3 && recs && ab && recs[0].ref == 0 && recs[0].won == 0 && ab[0].occ_common == 2 && ab[0].occ_won == 0 && ab[0].med_common == 2 && ab[0].med_won == 0 &&
          recs[1].won == 2 && ab[1].occ_common == 3 && ab[1].occ_won == 3 && ab[1].med_common == 1 && ab[1].med_won == 1 && ab[2].occ_won == 5 && ab[2].med_won == 5);
    CHECK(occ[0] == 4 && occ[1] == 3 && occ[2] == 3 && occ[3] == 5 && occ[4] == 5 && occ[5] == 5);
    rk_free_host(recs);
    rk_free_host(ab);
    // no query; no list
    uint64_t none[1] = {0}, out0[1] = {kMark};
    CHECK(rk_screen_abund_lists(nullptr, nullptr, 0, none, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, &o, out0, &recs, &ab, &n, nullptr, nullptr, nullptr, nullptr) ==
              RK_OK && out0[0] == 0 && recs == nullptr && ab == nullptr && n == 0);
    const uint64_t empties[3] = {0, 0, 0};
    CHECK(rk_screen_abund_lists(nullptr, nullptr, 0, empties, nullptr, nullptr, 2, 2, sizes, qsizes, qocc, &o, off, &recs, &ab, &n, matched, n_cand, claimed, occ) == RK_OK &&
          off[2] == 0 && matched[0] == 0 && recs == nullptr && ab == nullptr && occ[0] == 4 && occ[1] == 0 && occ[3] == 5 && occ[5] == 0);
    CHECK(rk_screen_abund_rows(nullptr, nullptr, nullptr, &o, off, &recs, &ab, &n, matched, n_cand, claimed, occ, nullptr) == RK_ERR_ARG);
#undef LISTS
}

// ---- rk_mask_lists_counts ---------------------------------------------------------------------------------------------------
template <class Hash> struct MaskCase {
    std::vector<Hash> q, lists;               // the query hashes back to back; the distinct hashes of the index, ascending
    std::vector<uint32_t> qc, lens;           // a count per query hash; the length of every list
    std::vector<uint64_t> off;                // n_query + 1
};

static unsigned long long n_mask_calls = 0;

template <class Hash> static void run_mask(const MaskCase<Hash> &c, const rk_mask_rule &rule)
{
    const uint32_t nq = (uint32_t)c.off.size() - 1;
    std::map<Hash, uint32_t> holders;
    for (size_t u = 0; u < c.lists.size(); u++) holders[c.lists[u]] = c.lens[u];
    std::vector<Hash> want;
    std::vector<uint32_t> want_c;
    std::vector<uint64_t> want_off{0};
    uint64_t matched = 0;
    uint32_t emptied = 0;
    for (uint32_t i = 0; i < nq; i++) {
        for (uint64_t j = c.off[i]; j < c.off[i + 1]; j++) {
            const auto it = holders.find(c.q[j]);
            const uint32_t n = it == holders.end() ? 0 : it->second;
            matched += n > 0;
            if (n >= rule.min_refs && n <= rule.max_refs) {
                want.push_back(c.q[j]);
                want_c.push_back(c.qc[j]);
            }
        }
        emptied += c.off[i + 1] > c.off[i] && want.size() == want_off.back();
        want_off.push_back(want.size());
    }
    const int wide = sizeof(Hash) == 8;
    std::vector<uint64_t> off((size_t)nq + 1, kMark), off2((size_t)nq + 1, kMark);
    void *h = (void *)(uintptr_t)kMark, *h2 = nullptr;
    uint32_t *kc = (uint32_t *)(uintptr_t)kMark;
    rk_mask_stats st, st2;
    memset(&st, 0x5A, sizeof st);
    memset(&st2, 0x5A, sizeof st2);
    n_mask_calls++;
    const void *Q = c.q.empty() ? nullptr : c.q.data(), *L = c.lists.empty() ? nullptr : c.lists.data();
    const uint32_t *QC = c.qc.empty() ? nullptr : c.qc.data(), *LN = c.lens.empty() ? nullptr : c.lens.data();
    const int rc = rk_mask_lists_counts(Q, QC, wide, c.off.data(), nq, L, LN, c.lists.size(), &rule, &h, &kc, off.data(), &st);
    CHECK(rc == RK_OK);
    if (rc != RK_OK) return;
    CHECK(off == want_off && (h == nullptr) == want.empty() && (kc == nullptr) == want.empty());
    CHECK(want.empty() || (!memcmp(h, want.data(), want.size() * sizeof(Hash)) && !memcmp(kc, want_c.data(), want.size() * 4)));
    CHECK(st.kept == want.size() && st.matched == matched && st.emptied == emptied && st.hashes == c.q.size() && st.path == 2);
    // hashes, offsets and statistics: byte for byte those of rk_mask_lists
    CHECK(rk_mask_lists(Q, wide, c.off.data(), nq, L, LN, c.lists.size(), &rule, &h2, off2.data(), &st2) == RK_OK);
    CHECK(off2 == off && !memcmp(&st, &st2, sizeof st) && (h2 == nullptr) == (h == nullptr) && (!h || !memcmp(h, h2, want.size() * sizeof(Hash))));
    rk_free_host(h);
    rk_free_host(h2);
    rk_free_host(kc);
}

template <class Hash> static unsigned long long mask_small_cases()
{
    unsigned long long seen = 0;
    const Hash base = sizeof(Hash) == 8 ? (Hash)0xFFFFFFFF0ULL : (Hash)3;   // (64 bits: hashes beyond 32 bits)
    for (uint32_t a = 0; a < 32; a++)
        for (uint32_t b = a; b < 33; b++) {   // b == 32: one reference; a == b == 0: none holds anything
            MaskCase<Hash> c;
            for (uint32_t x = 0; x < 5; x++) {
                const uint32_t n = (a >> x & 1) + (b < 32 ? b >> x & 1 : 0);
                if (n) {
                    c.lists.push_back(base + x);
                    c.lens.push_back(n);
                }
            }
            c.off.push_back(0);
            for (uint32_t m = 0; m < 32; m++) {   // every query over the 5 hashes and one nobody indexes, descending: any order goes
                c.q.push_back(base + 7);
                c.qc.push_back(0xFFFFFFFFu - m);
                for (int x = 4; x >= 0; x--)
                    if (m >> x & 1) {
                        c.q.push_back(base + (uint32_t)x);
                        c.qc.push_back(1 + (m * 5 + (uint32_t)x + a) % 7);
                    }
                c.off.push_back(c.q.size());
            }
            for (uint32_t lo = 0; lo < 4; lo++)
                for (uint32_t hi = lo; hi < 4; hi++) run_mask(c, rk_mask_rule{lo, hi});
            run_mask(c, rk_mask_rule{1, 0xFFFFFFFFu});
            seen++;
        }
    return seen;
}

template <class Hash> static void mask_random_cases(std::mt19937_64 &rng, int n_cases)
{
    const uint64_t space = sizeof(Hash) == 8 ? (1ULL << 36) : (1ULL << 24);
    for (int t = 0; t < n_cases; t++) {
        MaskCase<Hash> c;
        std::set<Hash> distinct;
        std::vector<Hash> pool;
        for (int i = 0, n = (int)(rng() % 40); i < n; i++) pool.push_back((Hash)(rng() % space));
        for (const Hash x : pool)
            if (rng() % 3) distinct.insert(x);
        for (const Hash x : distinct) {
            c.lists.push_back(x);
            c.lens.push_back((uint32_t)(rng() % 5));   // (an exported list may be empty)
        }
        c.off.push_back(0);
        for (int i = 0, n = (int)(rng() % 6); i < n; i++) {
            for (int j = 0, m = (int)(rng() % 30) * (int)(rng() % 4 != 0); j < m; j++) {
                c.q.push_back(!pool.empty() && rng() % 4 ? pool[rng() % pool.size()] : (Hash)(rng() % space));   // any order, repeats
                c.qc.push_back(rng() % 8 ? 1 + (uint32_t)(rng() % 9) : 0xFFFFFFFFu - (uint32_t)(rng() % 3));
            }
            c.off.push_back(c.q.size());
        }
        const uint32_t lo = (uint32_t)(rng() % 4), hi = rng() % 3 ? lo + (uint32_t)(rng() % 4) : 0xFFFFFFFFu;
        run_mask(c, rk_mask_rule{lo, hi});
    }
}

static void mask_refusals()
{
    const uint32_t q[2] = {5, 9}, qc[2] = {2, 3}, lists[1] = {5}, lens[1] = {1}, unsorted[2] = {9, 5}, two[2] = {1, 1};
    const uint64_t off[2] = {0, 2}, late[2] = {1, 2}, back[3] = {0, 2, 1};
    const rk_mask_rule sub{0, 0}, bad{2, 1};
    uint64_t out[3] = {kMark, kMark, kMark};
    void *h = (void *)(uintptr_t)kMark;
    uint32_t *kc = (uint32_t *)(uintptr_t)kMark;
#define MASK(Q, QC, OFF, NQ, L, LN, NL, R, H, KC, OUT) rk_mask_lists_counts(Q, QC, 0, OFF, NQ, L, LN, NL, R, H, KC, OUT, nullptr)
    CHECK(MASK(nullptr, qc, off, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, nullptr, off, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_ERR_ARG);      // hashes without their counts
    CHECK(MASK(q, qc, nullptr, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, nullptr, lens, 1, &sub, &h, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, lists, nullptr, 1, &sub, &h, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, lists, lens, 1, nullptr, &h, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, lists, lens, 1, &sub, nullptr, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, lists, lens, 1, &sub, &h, nullptr, out) == RK_ERR_ARG);       // no place for the counts
    CHECK(MASK(q, qc, off, 1, lists, lens, 1, &sub, &h, &kc, nullptr) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, lists, lens, 1, &bad, &h, &kc, out) == RK_ERR_ARG);           // min_refs above max_refs
    CHECK(MASK(q, qc, late, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_ERR_ARG);          // offsets that do not start at 0, that descend
    CHECK(MASK(q, qc, back, 2, lists, lens, 1, &sub, &h, &kc, out) == RK_ERR_ARG);
    CHECK(MASK(q, qc, off, 1, unsorted, two, 2, &sub, &h, &kc, out) == RK_ERR_ARG);         // list hashes that do not ascend
    CHECK(h == (void *)(uintptr_t)kMark && kc == (uint32_t *)(uintptr_t)kMark && out[0] == kMark && out[1] == kMark);
    CHECK(MASK(q, qc, off, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_OK && out[0] == 0 && out[1] == 1 && h && kc && ((uint32_t *)h)[0] == 9 && kc[0] == 3);
    rk_free_host(h);
    rk_free_host(kc);
    // nothing survives: no arrays; no hash at all; no query
    const uint32_t only[1] = {5}, c7[1] = {7};
    const uint64_t one[2] = {0, 1}, empty[2] = {0, 0}, none[1] = {0};
    CHECK(MASK(only, c7, one, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_OK && h == nullptr && kc == nullptr && out[1] == 0);
    CHECK(MASK(nullptr, nullptr, empty, 1, lists, lens, 1, &sub, &h, &kc, out) == RK_OK && h == nullptr && kc == nullptr && out[1] == 0);
    CHECK(MASK(nullptr, nullptr, none, 0, nullptr, nullptr, 0, &sub, &h, &kc, out) == RK_OK && h == nullptr && kc == nullptr && out[0] == 0);
    CHECK(rk_sketches_mask_counts(nullptr, nullptr, nullptr, &sub, nullptr, nullptr) == RK_ERR_ARG);
#undef MASK
}

int main()
{
    unsigned long long seen = 0;
    std::mt19937_64 rng(20261021);
    for (uint32_t n_ref = 1; n_ref <= 3; n_ref++) seen += small_cases(n_ref, rng);
    random_cases(rng, 2000);
    beyond_32_bits();
    refusals();
    const unsigned long long mask_seen = mask_small_cases<uint32_t>() + mask_small_cases<uint64_t>();
    mask_random_cases<uint32_t>(rng, 1000);
    mask_random_cases<uint64_t>(rng, 1000);
    mask_refusals();
    if (failures) {
        fprintf(stderr, "screen_abund_check: %d check(s) FAILED\n", failures);
        return 1;
    }
    printf("screen_abund_check: ok (screen: %llu small collections under 4 options each, 2000 random cases under every row shard, sums beyond 2^32, the empty cases "
           "and the refusals: %llu calls; mask: %llu small collections under 11 bands each, 2000 random cases, the empty cases and the refusals: %llu calls)\n",
           seen, n_calls, mask_seen, n_mask_calls);
    return 0;
}
