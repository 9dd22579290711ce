// Developer check: rk_screen_lists (host code of rk_screen.hip) against a plain restatement of the rule under the host sanitizers, as a
// stand-alone program -- EVERY collection of 1 .. 4 references and a query (with a second query of every other list) over a universe of
// 5 hashes under each of the 9 options min_common 1 .. 3 x min_won 0 .. 2, up to what cannot matter: the query is the first k hashes,
// the collection the multiset of their holder sets times, per reference, the number of hashes it holds outside the query
// (tests/test_screen_cpu.py says why that loses nothing), 32 references' worth of collections per call; 2,000 random cases of up to 12
// references with caller-given sizes, lists with repeats in any order and every row shard of 1 .. 3; products that differ by one next
// to the limit of the sizes; the empty cases and the refusals, none of which may write.
// The restatement ranks the candidates of a row once (std::sort) and gives a list to its member of the smallest rank; the library scans
// every list with the comparator.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_screen.hip -x hip tools/screen_lists_check.cpp -o screen_lists_check && ./screen_lists_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    std::vector<uint32_t> postings, counts, ref_sizes, query_sizes;
    std::vector<uint64_t> q_off, q_lists;
};

struct Cand {
    uint32_t common, size, ref;
};
// a comes before b: the larger common / size (products of 64 bits), then the larger size, then the smaller index
static bool before(const Cand &a, const Cand &b)
{
    const uint64_t ab = (uint64_t)a.common * b.size, ba = (uint64_t)b.common * a.size;
    if (ab != ba) return ab > ba;
    if (a.size != b.size) return a.size > b.size;
    return a.ref < b.ref;
}

static void run_case(const Case &c, const rk_screen_opts &o)
{
    const uint32_t nq = (uint32_t)c.q_off.size() - 1, n_ref = (uint32_t)c.ref_sizes.size();
    if (n_ref > 32) abort();
    std::vector<uint64_t> pos(c.counts.size() + 1, 0);
    for (size_t u = 0; u < c.counts.size(); u++) pos[u + 1] = pos[u] + c.counts[u];
    const uint32_t rb = o.row_block ? o.row_block : 1, rs = o.row_step ? o.row_step : 1;
    std::vector<rk_screen_rec> want;
    std::vector<uint64_t> want_off{0};
    std::vector<uint32_t> want_matched(nq, kMark32), want_cand(nq, kMark32), want_claimed(nq, kMark32);
    for (uint32_t q = 0; q < nq; q++) {
        if (q / rb >= o.row_first && (q / rb - o.row_first) % rs == 0) {
            std::vector<uint32_t> holders;   // per list of the query the set of its references, as bits (n_ref <= 32)
            std::vector<uint32_t> common(n_ref, 0), won(n_ref, 0), rank(n_ref, 0xFFFFFFFFu);
            uint32_t matched = 0, claimed = 0;
            for (uint64_t j = c.q_off[q]; j < c.q_off[q + 1]; j++) {
                const uint64_t u = c.q_lists[j];
                uint32_t bits = 0;
                for (uint64_t i = pos[u]; i < pos[u + 1]; i++) bits |= 1u << c.postings[i];   // repeats counted once
                holders.push_back(bits);
                matched += bits != 0;
                for (uint32_t r = 0; r < n_ref; r++) common[r] += bits >> r & 1;
            }
            std::vector<Cand> cands;
            for (uint32_t r = 0; r < n_ref; r++)
                if (common[r] >= o.min_common) cands.push_back(Cand{common[r], c.ref_sizes[r], r});
            std::sort(cands.begin(), cands.end(), before);
            for (size_t i = 0; i < cands.size(); i++) rank[cands[i].ref] = (uint32_t)i;
            for (const uint32_t bits : holders) {
                uint32_t best = 0xFFFFFFFFu;
                for (uint32_t r = 0; r < n_ref; r++)
                    if (bits >> r & 1) best = std::min(best, rank[r]);
                if (best != 0xFFFFFFFFu) {
                    won[cands[best].ref]++;
                    claimed++;
                }
            }
            for (uint32_t r = 0; r < n_ref; r++)
                if (common[r] >= o.min_common && won[r] >= o.min_won) want.push_back(rk_screen_rec{q, r, common[r], won[r], c.ref_sizes[r], c.query_sizes[q]});
            want_matched[q] = matched;
            want_cand[q] = (uint32_t)cands.size();
            want_claimed[q] = claimed;
            if (o.min_common == 1) CHECK(claimed == matched);
            if (!cands.empty()) CHECK(won[cands[0].ref] == cands[0].common);   // the best candidate keeps everything it shares
        }
        want_off.push_back(want.size());
    }
    std::vector<uint64_t> off((size_t)nq + 1, kMark);
    std::vector<uint32_t> matched(nq, kMark32), n_cand(nq, kMark32), claimed(nq, kMark32);
    rk_screen_rec *recs = (rk_screen_rec *)(uintptr_t)kMark;
    uint64_t n = kMark;
    n_calls++;
    const int rc = rk_screen_lists(c.postings.empty() ? nullptr : c.postings.data(), c.counts.empty() ? nullptr : c.counts.data(), c.counts.size(), c.q_off.data(),
                                   c.q_lists.empty() ? nullptr : c.q_lists.data(), nq, n_ref, n_ref ? c.ref_sizes.data() : nullptr, nq ? c.query_sizes.data() : nullptr,
                                   &o, off.data(), &recs, &n, nq ? matched.data() : nullptr, nq ? n_cand.data() : nullptr, nq ? claimed.data() : nullptr);
    CHECK(rc == RK_OK);
    if (rc != RK_OK) return;
    CHECK(off == want_off && n == want.size() && (recs == nullptr) == want.empty());
    CHECK(want.empty() || !memcmp(recs, want.data(), want.size() * sizeof(rk_screen_rec)));
    CHECK(matched == want_matched && n_cand == want_cand && claimed == want_claimed);   // (the entries of unselected rows keep their mark)
    rk_free_host(recs);
}

// Several small collections in ONE call per option (every call costs a dozen allocations under the sanitizer): a collection keeps its
// lists to itself, its references and queries follow those of the collections before it -- a tie goes by the index, and the order within
// a collection is kept.  run(): the 9 options min_common 1 .. 3 x min_won 0 .. 2.
struct Together {
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
        for (const uint64_t u : c.q_lists) all.q_lists.push_back(u + u0);
        for (size_t q = 1; q < c.q_off.size(); q++) all.q_off.push_back(c.q_off[q] + j0);
        n++;
    }
    void run()
    {
        if (!n) return;
        for (uint32_t mc = 1; mc <= 3; mc++)
            for (uint32_t mw = 0; mw <= 2; mw++) run_case(all, rk_screen_opts{mc, mw, 0, 0, 0});
        all = Case();
        n = 0;
    }
};

// every collection of n_ref references over 5 hashes, by holder sets and sizes, each under the 9 options
static unsigned long long small_cases(uint32_t n_ref)
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
                together.add(c);
                if (together.n == 32 / n_ref) together.run();   // (the restatement keeps a list's holders in 32 bits)
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
            // the next multiset
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
        for (uint32_t r = 0; r < N; r++) c.ref_sizes.push_back(held[r] + (uint32_t)(rng() % 4) * (uint32_t)(rng() % 3));   // at least what it can share; ties are common
        c.q_off.push_back(0);
        for (int i = 0, n = (int)(rng() % 7); i < n; i++) {
            std::set<uint64_t> mine;
            for (int j = 0, m = n_lists ? (int)(rng() % 20) * (int)(rng() % 3 != 0) : 0; j < m; j++) mine.insert(rng() % n_lists);
            c.q_lists.insert(c.q_lists.end(), mine.begin(), mine.end());   // strictly ascending
            c.q_off.push_back(c.q_lists.size());
            c.query_sizes.push_back((uint32_t)mine.size() + (uint32_t)(rng() % 5));
        }
        const uint32_t mc = (uint32_t)(rng() % 3) + 1, mw = (uint32_t)(rng() % 3);
        run_case(c, rk_screen_opts{mc, mw, 0, 0, 0});
        const uint32_t step = (uint32_t)(rng() % 3) + 1;
        for (uint32_t first = 0; first < step; first++) run_case(c, rk_screen_opts{mc, mw, first, step, (uint32_t)(rng() % 3)});
    }
}

// reference 0 holds the L lists of the query, reference 1 all but the last; the sizes make the two products differ by one, either way
static void near_the_limit()
{
    const uint32_t L = (1u << 10) + 1;
    Case c;
    for (uint32_t u = 0; u < L; u++) {
        c.postings.push_back(0);
        if (u + 1 < L) c.postings.push_back(1);
        c.counts.push_back(u + 1 < L ? 2 : 1);
        c.q_lists.push_back(u);
    }
    c.q_off = {0, L};
    c.query_sizes = {L};
    for (const uint32_t m : {1047551u, 1000003u, 999u}) {
        for (const int d : {1, -1}) {
            c.ref_sizes = {(uint32_t)((int64_t)L * m + d), (uint32_t)((int64_t)m * (L - 1) + d)};
            CHECK(c.ref_sizes[0] < (1u << 30) && (int64_t)L * c.ref_sizes[1] - (int64_t)(L - 1) * c.ref_sizes[0] == d);
            run_case(c, rk_screen_opts{1, 0, 0, 0, 0});
            uint64_t off[2], n = 0;
            uint32_t matched, n_cand, claimed;
            rk_screen_rec *recs = nullptr;
            const rk_screen_opts o{1, 0, 0, 0, 0};
            CHECK(rk_screen_lists(c.postings.data(), c.counts.data(), L, c.q_off.data(), c.q_lists.data(), 1, 2, c.ref_sizes.data(), c.query_sizes.data(), &o, off, &recs,
                                  &n, &matched, &n_cand, &claimed) == RK_OK);
            CHECK(n == 2 && recs && recs[0].won == (d == 1 ? L : 1) && recs[1].won == (d == 1 ? 0 : L - 1) && claimed == L);   // worked by hand
            rk_free_host(recs);
        }
    }
}

static void refusals()
{
    const uint32_t postings[3] = {0, 1, 1}, counts[2] = {2, 1}, sizes[2] = {1, 2}, qsizes[2] = {2, 1}, bad_post[3] = {0, 2, 1}, small[2] = {1, 1};
    const uint32_t huge[2] = {1, 1u << 30}, qhuge[2] = {1u << 30, 1}, largest[2] = {1, (1u << 30) - 1};
    const uint64_t q_off[3] = {0, 2, 3}, ql[3] = {0, 1, 1}, late[3] = {1, 2, 3}, back[3] = {0, 3, 2}, far[3] = {0, 2, 1}, down[3] = {1, 0, 1}, twice[3] = {0, 0, 1};
    const rk_screen_opts o{1, 0, 0, 0, 0}, zero{0, 0, 0, 0, 0}, second_row{1, 0, 1, 2, 1};
    uint64_t off[3] = {kMark, kMark, kMark}, n = kMark;
    uint32_t matched[2] = {kMark32, kMark32}, n_cand[2] = {kMark32, kMark32}, claimed[2] = {kMark32, kMark32};
    rk_screen_rec *recs = (rk_screen_rec *)(uintptr_t)kMark;
#define LISTS(P, C, QO, QL, S, Z, O, OFF, R, N, M, K, W) rk_screen_lists(P, C, 2, QO, QL, 2, 2, S, Z, O, OFF, R, N, M, K, W)
    CHECK(LISTS(nullptr, counts, q_off, ql, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, nullptr, q_off, ql, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, nullptr, ql, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, nullptr, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, nullptr, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, nullptr, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, nullptr, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &o, nullptr, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &o, off, nullptr, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &o, off, &recs, nullptr, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &o, off, &recs, &n, nullptr, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &o, off, &recs, &n, matched, nullptr, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, nullptr) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qsizes, &zero, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    for (const uint64_t *qo : {late, back}) CHECK(LISTS(postings, counts, qo, ql, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    for (const uint64_t *l : {far, down, twice}) CHECK(LISTS(postings, counts, q_off, l, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(bad_post, counts, q_off, ql, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, small, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);   // reference 1 shares 2 hashes with query 0
    CHECK(LISTS(postings, counts, q_off, ql, huge, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, sizes, qhuge, &o, off, &recs, &n, matched, n_cand, claimed) == RK_ERR_ARG);
    CHECK(recs == (rk_screen_rec *)(uintptr_t)kMark && n == kMark && off[0] == kMark && off[2] == kMark && matched[0] == kMark32 && n_cand[1] == kMark32 &&
          claimed[0] == kMark32);
    // the good call writes, at the largest size there is: list 0 is held by 0 and 1, list 1 by 1 alone; 1/1 beats 2/(2^30 - 1)
    CHECK(LISTS(postings, counts, q_off, ql, largest, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_OK);
    CHECK(off[0] == 0 && off[1] == 2 && off[2] == 3 && n == 3 && recs && recs[0].ref == 0 && recs[0].won == 1 && recs[1].ref == 1 && recs[1].common == 2 &&
          recs[1].won == 1 && recs[1].size_ref == (1u << 30) - 1 && recs[2].query == 1 && recs[2].won == 1 && matched[0] == 2 && claimed[1] == 1);
    rk_free_host(recs);
    // only the selected rows are read: row 1 alone is fine under sizes that row 0 breaks
    CHECK(LISTS(postings, counts, q_off, ql, small, qsizes, &second_row, off, &recs, &n, matched, n_cand, claimed) == RK_OK && n == 1 && off[1] == 0 && off[2] == 1);
    rk_free_host(recs);
    // no query; no list; no reference
    uint64_t none[1] = {0}, out0[1] = {kMark};
    CHECK(rk_screen_lists(nullptr, nullptr, 0, none, nullptr, 0, 0, nullptr, nullptr, &o, out0, &recs, &n, nullptr, nullptr, nullptr) == RK_OK && out0[0] == 0 &&
          recs == nullptr && n == 0);
    const uint64_t empties[3] = {0, 0, 0};
    CHECK(rk_screen_lists(nullptr, nullptr, 0, empties, nullptr, 2, 2, sizes, qsizes, &o, off, &recs, &n, matched, n_cand, claimed) == RK_OK && off[2] == 0 &&
          matched[0] == 0 && n_cand[1] == 0 && claimed[1] == 0 && recs == nullptr);
    CHECK(rk_screen_rows(nullptr, nullptr, nullptr, &o, off, &recs, &n, matched, n_cand, claimed, nullptr) == RK_ERR_ARG);
#undef LISTS
}

int main()
{
    unsigned long long seen = 0;
    for (uint32_t n_ref = 1; n_ref <= 4; n_ref++) seen += small_cases(n_ref);
    std::mt19937_64 rng(20261021);
    random_cases(rng, 2000);
    near_the_limit();
    refusals();
    if (failures) {
        fprintf(stderr, "screen_lists_check: %d check(s) FAILED\n", failures);
        return 1;
    }
    printf("screen_lists_check: ok (%llu small collections under 9 options each, 2000 random cases under every row shard, products one apart, the empty cases and the "
           "refusals: %llu calls)\n", seen, n_calls);
    return 0;
}
