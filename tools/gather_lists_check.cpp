// Developer check: rk_gather_lists (host code of rk_gather.hip) against a plain restatement of the rule under the host sanitizers, as a
// stand-alone program -- 2,000 random small collections (1 .. 14 references, up to 24 posting lists in shuffled order with repeated
// references and empty lists, 1 .. 5 queries of up to 24 lists, min_new 1 .. 5, max_picks 0 .. 3, row shards), the cases without a
// query, a list or a reference, and the refusals (min_new 0, offsets that do not ascend from 0, a list that does not exist or comes out
// of order, a posting beyond the references, null pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_gather.hip -x hip tools/gather_lists_check.cpp -o gather_lists_check && ./gather_lists_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>
#include "rk_internal.h"
// what rk_gather.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
int rk_read_back(rk_ctx *, void *, const void *, size_t, hipStream_t) { return -1; }
int rk_index_ensure_dir(rk_ctx *, rk_index *, hipStream_t) { return -1; }
int rk_distq_counts(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, uint32_t, uint32_t, int32_t *, hipStream_t) { return -1; }
extern "C" int rk_index_export_lists(const rk_index *, uint32_t *, uint32_t *, uint32_t *) { return -1; }
extern "C" int rk_index_export64(const rk_index *, uint32_t *, uint64_t *, uint32_t *) { return -1; }
extern "C" int rk_index_order(const rk_index *, uint32_t *) { return -1; }
extern "C" int rk_sketches_download(const rk_sketches *, uint32_t *, uint64_t *) { return -1; }
extern "C" int rk_sketches_download64(const rk_sketches *, uint64_t *, uint64_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

struct Pick {
    uint32_t w[8];
    bool operator==(const Pick &o) const { return !memcmp(w, o.w, sizeof w); }
};
struct Result {
    std::vector<uint64_t> off;
    std::vector<Pick> picks;
    std::vector<uint32_t> matched, n_cand, covered;
    bool operator==(const Result &o) const { return off == o.off && picks == o.picks && matched == o.matched && n_cand == o.n_cand && covered == o.covered; }
};
static const uint32_t kMark = 0x5A5A5A5Au;

static bool selected(uint32_t q, const rk_gather_opts &o)
{
    const uint32_t rb = o.row_block ? o.row_block : 1, rs = o.row_step ? o.row_step : 1, blk = q / rb;
    return blk >= o.row_first && (blk - o.row_first) % rs == 0;
}

// the rule, plainly: sets, the remaining intersections recomputed in every round
static Result plain(const std::vector<std::vector<uint32_t>> &lists, const std::vector<std::vector<uint64_t>> &queries, uint32_t n_ref,
                    const std::vector<uint32_t> &ref_sizes, const std::vector<uint32_t> &query_sizes, const rk_gather_opts &o)
{
    Result out;
    const uint32_t Q = (uint32_t)queries.size();
    out.off.push_back(0);
    out.matched.assign(Q, kMark);
    out.n_cand.assign(Q, kMark);
    out.covered.assign(Q, kMark);
    for (uint32_t q = 0; q < Q; q++) {
        if (selected(q, o)) {
            std::set<uint64_t> M;
            for (uint64_t u : queries[q])
                if (!lists[u].empty()) M.insert(u);
            std::vector<std::set<uint64_t>> of(n_ref);   // per reference the query's lists that name it
            for (uint64_t u : M)
                for (uint32_t r : lists[u]) of[r].insert(u);
            uint32_t n_cand = 0, covered = 0, t = 0;
            for (uint32_t r = 0; r < n_ref; r++) n_cand += of[r].size() >= o.min_new;
            out.matched[q] = (uint32_t)M.size();
            std::set<uint32_t> picked;
            while (!o.max_picks || t < o.max_picks) {
                uint32_t best = 0, best_ref = 0;
                for (uint32_t r = 0; r < n_ref; r++) {
                    if (picked.count(r)) continue;
                    uint32_t rem = 0;
                    for (uint64_t u : of[r]) rem += (uint32_t)M.count(u);
                    if (rem > best) {
                        best = rem;
                        best_ref = r;
                    }
                }
                if (best < o.min_new) break;
                for (uint64_t u : of[best_ref]) M.erase(u);
                picked.insert(best_ref);
                covered += best;
                out.picks.push_back(Pick{{q, best_ref, t, (uint32_t)of[best_ref].size(), best, (uint32_t)M.size(), ref_sizes[best_ref], query_sizes[q]}});
                t++;
            }
            out.n_cand[q] = n_cand;
            out.covered[q] = covered;
        }
        out.off.push_back(out.picks.size());
    }
    return out;
}

struct Call {
    std::vector<uint64_t> off;
    std::vector<uint32_t> matched, n_cand, covered;
    rk_gather_pick *picks = (rk_gather_pick *)0x10;
    uint64_t n = 77;
    explicit Call(uint32_t Q) : off((size_t)Q + 1, kMark), matched(Q, kMark), n_cand(Q, kMark), covered(Q, kMark) {}
    bool untouched() const
    {
        auto marked = [](const auto &v) { return std::all_of(v.begin(), v.end(), [](auto x) { return x == kMark; }); };
        return picks == (rk_gather_pick *)0x10 && n == 77 && marked(off) && marked(matched) && marked(n_cand) && marked(covered);
    }
};

struct Flat {
    std::vector<uint32_t> postings, counts;
    std::vector<uint64_t> q_off, q_lists;
    Flat(const std::vector<std::vector<uint32_t>> &lists, const std::vector<std::vector<uint64_t>> &queries)
    {
        for (const auto &l : lists) {
            postings.insert(postings.end(), l.begin(), l.end());
            counts.push_back((uint32_t)l.size());
        }
        q_off.push_back(0);
        for (const auto &q : queries) {
            q_lists.insert(q_lists.end(), q.begin(), q.end());
            q_off.push_back(q_lists.size());
        }
    }
};

static int call(const Flat &f, uint32_t n_ref, const std::vector<uint32_t> &ref_sizes, const std::vector<uint32_t> &query_sizes, const rk_gather_opts *o, Call *c)
{
    return rk_gather_lists(f.postings.data(), f.counts.data(), f.counts.size(), f.q_off.data(), f.q_lists.data(), (uint32_t)query_sizes.size(), n_ref,
                           ref_sizes.data(), query_sizes.data(), o, c->off.data(), &c->picks, &c->n, c->matched.data(), c->n_cand.data(), c->covered.data());
}

static Result taken(Call &c)
{
    Result r;
    r.off = c.off;
    static_assert(sizeof(Pick) == sizeof(rk_gather_pick), "a pick is eight words");
    r.picks.resize(c.n);
    if (c.n) memcpy(r.picks.data(), c.picks, c.n * sizeof(Pick));
    r.matched = c.matched;
    r.n_cand = c.n_cand;
    r.covered = c.covered;
    rk_free_host(c.picks);
    return r;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
    std::mt19937 rng(20261020);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    unsigned long long picks = 0, many = 0, stopped = 0, unsorted = 0;
    for (int it = 0; it < 2000; it++) {
        const uint32_t n_ref = 1 + below(14), n_lists = below(25), Q = 1 + below(5);
        std::vector<std::vector<uint32_t>> lists(n_lists);
        const bool tidy = it % 3 == 0;   // every list strictly ascending: rk_gather_lists then reads the caller's arrays in place
        for (auto &l : lists) {
            l.resize(it % 4 < 2 ? below(3) : below(n_ref + 3));   // (an empty list may stand in the middle; repeats happen; short lists: many picks)
            for (auto &v : l) v = below(n_ref);
            if (tidy) {
                std::sort(l.begin(), l.end());
                l.erase(std::unique(l.begin(), l.end()), l.end());
            }
        }
        unsorted += !tidy;
        std::vector<std::vector<uint64_t>> queries(Q);
        for (auto &q : queries)
            for (uint64_t u = 0; u < n_lists; u++)
                if (below(3)) q.push_back(u);
        std::vector<uint32_t> ref_sizes(n_ref), query_sizes(Q);
        for (auto &s : ref_sizes) s = below(1000);
        for (auto &s : query_sizes) s = below(1000);
        rk_gather_opts o = {1 + below(5) * (uint32_t)(it % 2), it % 2 ? below(4) : 0u, 0, 0, 0};   // every other case: the whole cover
        if (it % 7 == 6) o = rk_gather_opts{1 + below(2), 0, below(2), 2, 1 + below(3)};
        const Flat f(lists, queries);
        Call c(Q);
        CHECK(call(f, n_ref, ref_sizes, query_sizes, &o, &c) == RK_OK);
        for (uint32_t q = 0; q < Q; q++)   // entries of unselected rows are not written
            CHECK(selected(q, o) ? c.matched[q] != kMark : (c.matched[q] == kMark && c.n_cand[q] == kMark && c.covered[q] == kMark));
        const Result got = taken(c), want = plain(lists, queries, n_ref, ref_sizes, query_sizes, o);
        CHECK(got == want);
        picks += got.picks.size();
        for (uint32_t q = 0; q < Q; q++) {
            many += got.off[q + 1] - got.off[q] > 3;
            stopped += o.max_picks && got.off[q + 1] - got.off[q] == o.max_picks;
            if (o.min_new == 1 && !o.max_picks && selected(q, o)) CHECK(got.covered[q] == got.matched[q]);
        }
    }
    CHECK(picks > 5000 && many > 300 && stopped > 300 && unsorted > 1000);
    const rk_gather_opts one = {1, 0, 0, 0, 0};
    {   // no query, no list, no reference
        const uint64_t zero = 0;
        Call d(0);
        CHECK(rk_gather_lists(nullptr, nullptr, 0, &zero, nullptr, 0, 0, nullptr, nullptr, &one, d.off.data(), &d.picks, &d.n, nullptr, nullptr, nullptr) == RK_OK);
        CHECK(d.n == 0 && !d.picks && d.off[0] == 0);
        Call e(2);   // two queries that hit nothing, against two references without a list
        const uint64_t qo[3] = {0, 0, 0};
        const uint32_t sizes[2] = {4, 5};
        CHECK(rk_gather_lists(nullptr, nullptr, 0, qo, nullptr, 2, 2, sizes, sizes, &one, e.off.data(), &e.picks, &e.n, e.matched.data(), e.n_cand.data(), e.covered.data()) == RK_OK);
        CHECK(e.n == 0 && !e.picks && e.off == std::vector<uint64_t>({0, 0, 0}) && e.matched == std::vector<uint32_t>({0, 0}) && e.covered == e.matched);
    }
    {   // the refusals write nothing
        const std::vector<std::vector<uint32_t>> lists = {{0, 1}, {1}};
        const std::vector<std::vector<uint64_t>> queries = {{0, 1}, {}};
        const std::vector<uint32_t> rs = {2, 1}, qs = {3, 0};
        const Flat f(lists, queries);
        Call c(2);
        const rk_gather_opts zero_new = {0, 0, 0, 0, 0};
        CHECK(call(f, 2, rs, qs, &zero_new, &c) == RK_ERR_ARG && call(f, 2, rs, qs, nullptr, &c) == RK_ERR_ARG);
        CHECK(call(Flat({{0, 2}, {1}}, queries), 2, rs, qs, &one, &c) == RK_ERR_ARG);          // a posting beyond the references
        CHECK(call(Flat(lists, {{0, 2}, {}}), 2, rs, qs, &one, &c) == RK_ERR_ARG);             // a list that does not exist
        CHECK(call(Flat(lists, {{1, 0}, {}}), 2, rs, qs, &one, &c) == RK_ERR_ARG);             // lists out of order
        CHECK(call(Flat(lists, {{1, 1}, {}}), 2, rs, qs, &one, &c) == RK_ERR_ARG);             // ... or twice
        Flat g(lists, queries);
        g.q_off = {1, 2, 2};
        CHECK(call(g, 2, rs, qs, &one, &c) == RK_ERR_ARG);                                       // offsets that do not begin at 0
        g.q_off = {0, 2, 1};
        CHECK(call(g, 2, rs, qs, &one, &c) == RK_ERR_ARG);                                       // ... that descend
        const uint32_t *P = f.postings.data(), *N = f.counts.data(), *RS = rs.data(), *QS = qs.data();
        const uint64_t *QO = f.q_off.data(), *QL = f.q_lists.data();
        uint64_t *off = c.off.data();
        uint32_t *m = c.matched.data(), *nc = c.n_cand.data(), *cv = c.covered.data();
        CHECK(rk_gather_lists(nullptr, N, 2, QO, QL, 2, 2, RS, QS, &one, off, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, nullptr, 2, QO, QL, 2, 2, RS, QS, &one, off, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, nullptr, QL, 2, 2, RS, QS, &one, off, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, nullptr, 2, 2, RS, QS, &one, off, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, nullptr, QS, &one, off, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, nullptr, &one, off, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, QS, &one, nullptr, &c.picks, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, QS, &one, off, nullptr, &c.n, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, QS, &one, off, &c.picks, nullptr, m, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, QS, &one, off, &c.picks, &c.n, nullptr, nc, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, QS, &one, off, &c.picks, &c.n, m, nullptr, cv) == RK_ERR_ARG);
        CHECK(rk_gather_lists(P, N, 2, QO, QL, 2, 2, RS, QS, &one, off, &c.picks, &c.n, m, nc, nullptr) == RK_ERR_ARG);
        CHECK(c.untouched());
        CHECK(rk_gather_rows(nullptr, nullptr, nullptr, &one, off, &c.picks, &c.n, m, nc, cv, nullptr) == RK_ERR_ARG && c.untouched());
        CHECK(call(f, 2, rs, qs, &one, &c) == RK_OK && c.n == 1 && c.picks[0].ref == 1 && c.picks[0].fresh == 2 && c.picks[0].left == 0);   // and the good call writes
        rk_free_host(c.picks);
    }
    printf("gather_lists_check: 2000 collections, %llu picks, %llu queries of more than 3 picks, %llu stopped by max_picks: ok\n", picks, many, stopped);
    return 0;
}
