// Developer check: rk_assign_hits (host code of rk_assign.hip) against a plain restatement of the rule under the host sanitizers, as a
// stand-alone program -- 600 random small record lists (1 .. 12 queries against 1 .. 24 references, both metrics, labels below the number
// of references that need not be members, unlabelled references, equal ratios from different counts), each also in shuffled record order
// and without the record arrays, and the refusals (a query or a reference beyond their number, a label that names nothing, a record
// outside 0 < common <= u, null pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_assign.hip -x hip tools/assign_hits_check.cpp -o assign_hits_check && ./assign_hits_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "rk_internal.h"
// what rk_assign.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
void *rk_pinned_scratch(rk_ctx *, size_t) { return nullptr; }
uint64_t rk_host_exact_distances(rk_hit *, uint64_t, const rk_dist_opts *) { return 0; }
extern "C" int rk_dist_rows_dev(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit *, uint64_t, uint64_t *, void *) { return -1; }
extern "C" int rk_dist_rows(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit **, uint64_t *, int32_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

static const int kTriples[5][3] = {{20, 50, 50}, {40, 60, 60}, {60, 70, 70}, {20, 40, 40}, {25, 50, 50}};   // 20/60 ties 25/75
static const uint32_t kNone = RK_ASSIGN_NONE;
static const rk_hit kMark = {77, 77, 77, 77, 77, 77, 7.0, 7.0};
static const rk_hit kAbsent = {kNone, kNone, 0, 0, 0, 0, 0.0, 0.0};

static bool same_hit(const rk_hit &a, const rk_hit &b) { return memcmp(&a, &b, sizeof a) == 0; }

struct Out {
    std::vector<uint32_t> label, n_within, n_labelled, n_same;
    std::vector<rk_hit> nearest, runner_up;
    explicit Out(uint32_t q) : label(q, 77), n_within(q, 77), n_labelled(q, 77), n_same(q, 77), nearest(q, kMark), runner_up(q, kMark) {}
    rk_assign_queries g(bool records = true)
    {
        return rk_assign_queries{label.data(), n_within.data(), n_labelled.data(), n_same.data(), records ? nearest.data() : nullptr,
                                 records ? runner_up.data() : nullptr};
    }
    bool counts_equal(const Out &o) const { return label == o.label && n_within == o.n_within && n_labelled == o.n_labelled && n_same == o.n_same; }
    bool operator==(const Out &o) const
    {
        return counts_equal(o) && std::equal(nearest.begin(), nearest.end(), o.nearest.begin(), same_hit) &&
               std::equal(runner_up.begin(), runner_up.end(), o.runner_up.begin(), same_hit);
    }
};

static long long u_of(const rk_hit &h, int metric) { return metric ? std::min(h.size0, h.size1) : (long long)h.size0 + h.size1 - h.common; }
// the sign of ratio(a) - ratio(b): integers only
static int cross(const rk_hit &a, const rk_hit &b, int metric)
{
    const long long l = a.common * u_of(b, metric), r = b.common * u_of(a, metric);
    return l < r ? -1 : l > r ? 1 : 0;
}

// the rule, plainly: per query two walks over every record
static Out plain(const std::vector<rk_hit> &hits, uint32_t n_query, const std::vector<uint32_t> &label, int metric)
{
    Out o(n_query);
    for (uint32_t q = 0; q < n_query; q++) {
        o.n_within[q] = o.n_labelled[q] = o.n_same[q] = 0;
        o.nearest[q] = o.runner_up[q] = kAbsent;
        for (const rk_hit &h : hits) {
            if (h.row != q) continue;
            o.n_within[q]++;
            if (label[h.col] == kNone) continue;
            o.n_labelled[q]++;
            const rk_hit &best = o.nearest[q];
            const int c = best.row == kNone ? 1 : cross(h, best, metric);
            if (c > 0 || (!c && h.col < best.col)) o.nearest[q] = h;
        }
        o.label[q] = o.nearest[q].row == kNone ? kNone : label[o.nearest[q].col];
        for (const rk_hit &h : hits) {
            if (h.row != q || label[h.col] == kNone) continue;
            if (label[h.col] == o.label[q]) {
                o.n_same[q]++;
                continue;
            }
            const rk_hit &best = o.runner_up[q];
            const int c = best.row == kNone ? 1 : cross(h, best, metric);
            if (c > 0 || (!c && h.col < best.col)) o.runner_up[q] = h;
        }
    }
    return o;
}

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                \
        }                                                            \
    } while (0)

int main()
{
    std::mt19937_64 rng(20261019);
    auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    unsigned long long ties = 0, seconds = 0, novel = 0;
    for (int round = 0; round < 600; round++) {
        const uint32_t n_query = 1 + below(12), n_ref = 1 + below(24);
        const int metric = round & 1;
        std::vector<uint32_t> label(n_ref);
        const uint32_t kinds = 1 + below(n_ref);
        for (uint32_t r = 0; r < n_ref; r++) label[r] = below(4) == 0 ? kNone : below(kinds) * (n_ref / kinds);   // (below n_ref, need not be a member)
        std::vector<rk_hit> hits;
        const uint32_t density = 1 + below(4);
        for (uint32_t q = 0; q < n_query; q++)
            for (uint32_t r = 0; r < n_ref; r++) {
                if (below(4) >= density) continue;
                const int *t = kTriples[below(5)];
                hits.push_back(rk_hit{q, r, t[0], t[1], t[2], 0, 0.25 + (double)hits.size(), 0.5 + (double)hits.size()});   // (jorc, dist: marks that must travel)
            }
        const Out want = plain(hits, n_query, label, metric);
        Out got(n_query);
        rk_assign_queries g = got.g();
        CHECK(rk_assign_hits(hits.data(), hits.size(), n_query, n_ref, label.data(), metric, &g) == RK_OK);
        CHECK(got == want);
        std::vector<rk_hit> shuffled = hits;
        std::shuffle(shuffled.begin(), shuffled.end(), rng);
        Out again(n_query);
        g = again.g();
        CHECK(rk_assign_hits(shuffled.data(), shuffled.size(), n_query, n_ref, label.data(), metric, &g) == RK_OK);
        CHECK(again == want);
        Out bare(n_query);
        g = bare.g(false);
        CHECK(rk_assign_hits(hits.data(), hits.size(), n_query, n_ref, label.data(), metric, &g) == RK_OK);
        CHECK(bare.counts_equal(want) && same_hit(bare.nearest[0], kMark) && same_hit(bare.runner_up[0], kMark));
        for (uint32_t q = 0; q < n_query; q++) {
            seconds += want.runner_up[q].row != kNone;
            novel += want.label[q] == kNone && want.n_within[q];
            if (want.nearest[q].row == kNone) continue;
            unsigned equal = 0;
            for (const rk_hit &h : hits) equal += h.row == q && label[h.col] != kNone && !cross(h, want.nearest[q], metric);
            ties += equal > 1;
        }
    }
    CHECK(ties > 300 && seconds > 1000 && novel > 100);   // what the rounds are for

    // the refusals: nothing is written
    const std::vector<uint32_t> label = {0, 0, 2, kNone};
    const std::vector<rk_hit> good = {{0, 1, 25, 50, 50, 0, 0.0, 0.0}, {2, 3, 20, 40, 40, 0, 0.0, 0.0}};
    Out out(3);
    const Out clean(3);
    rk_assign_queries g = out.g();
    const struct { rk_hit h; int code; } bad[] = {{{3, 1, 25, 50, 50, 0, 0.0, 0.0}, RK_ERR_ARG},          {{0, 4, 25, 50, 50, 0, 0.0, 0.0}, RK_ERR_ARG},
                                                   {{0, 2, 0, 50, 50, 0, 0.0, 0.0}, RK_ERR_UNSUPPORTED},   {{0, 2, 51, 50, 50, 0, 0.0, 0.0}, RK_ERR_UNSUPPORTED},
                                                   {{0, 2, -1, 50, 50, 0, 0.0, 0.0}, RK_ERR_UNSUPPORTED}};
    for (const auto &b : bad) {
        const std::vector<rk_hit> hits = {good[0], b.h};
        CHECK(rk_assign_hits(hits.data(), 2, 3, 4, label.data(), 1, &g) == b.code);
    }
    for (uint32_t wrong : {4u, kNone - 1}) {
        std::vector<uint32_t> l = label;
        l[1] = wrong;
        CHECK(rk_assign_hits(good.data(), 2, 3, 4, l.data(), 0, &g) == RK_ERR_ARG);
    }
    CHECK(rk_assign_hits(good.data(), 2, 3, 4, nullptr, 0, &g) == RK_ERR_ARG);
    CHECK(rk_assign_hits(nullptr, 2, 3, 4, label.data(), 0, &g) == RK_ERR_ARG);
    CHECK(rk_assign_hits(good.data(), 2, 3, 4, label.data(), 0, nullptr) == RK_ERR_ARG);
    for (int k = 0; k < 4; k++) {
        rk_assign_queries lone = out.g();
        (k == 0 ? lone.label : k == 1 ? lone.n_within : k == 2 ? lone.n_labelled : lone.n_same) = nullptr;
        CHECK(rk_assign_hits(good.data(), 2, 3, 4, label.data(), 0, &lone) == RK_ERR_ARG);
    }
    CHECK(out == clean);
    CHECK(rk_assign_hits(good.data(), 2, 3, 4, label.data(), 0, &g) == RK_OK);
    CHECK(out == plain(good, 3, label, 0));
    rk_assign_queries none{};
    CHECK(rk_assign_hits(nullptr, 0, 0, 0, nullptr, 0, &none) == RK_OK);   // no query: nothing to write
    printf("assign_hits_check: 600 rounds (%llu nearest records decided by a tie, %llu runner-ups, %llu novel queries with records) and the refusals: ok\n", ties,
           seconds, novel);
    return 0;
}
