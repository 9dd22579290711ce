// Developer check: rk_group_lists (host code of rk_group.hip) against a plain restatement of the rule under the host sanitizers, as a
// stand-alone program -- 2,000 random small collections (1 .. 12 genomes, up to 20 posting lists in shuffled order with repeated genomes,
// labels below the number of genomes that need not be members, unlabelled genomes, the four named rules and random ones), the cases
// without a group and without a list, and the refusals (a posting beyond the genomes, a label that names nothing, a bad rule, null
// pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_group.hip -x hip tools/group_lists_check.cpp -o group_lists_check && ./group_lists_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>
#include "rk_internal.h"
// what rk_group.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
int rk_read_back(rk_ctx *, void *, const void *, size_t, hipStream_t) { return -1; }
int rk_prim_sort_keys_u64(rk_ctx *, const unsigned long long *, unsigned long long *, uint64_t, unsigned, unsigned, hipStream_t, void **) { return -1; }
int rk_prim_rle_u64(rk_ctx *, const unsigned long long *, uint64_t, unsigned long long *, unsigned int *, unsigned long long *, hipStream_t) { return -1; }
extern "C" int rk_index_export_lists(const rk_index *, uint32_t *, uint32_t *, uint32_t *) { return -1; }
extern "C" int rk_index_export64(const rk_index *, uint32_t *, uint64_t *, uint32_t *) { return -1; }
extern "C" int rk_sketches_from_host(rk_ctx *, const uint32_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" int rk_sketches_from_host64(rk_ctx *, const uint64_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" void rk_sketches_free(rk_sketches *) {}
extern "C" void rk_free_host(void *p) { free(p); }

static const uint32_t kNone = RK_GROUP_NONE;

struct Result {
    std::vector<uint64_t> off, kept;
    std::vector<uint32_t> label, size;
    bool operator==(const Result &o) const { return off == o.off && kept == o.kept && label == o.label && size == o.size; }
};

// the rule, plainly: per label in use, per list, two counts over the set of its genomes
static Result plain(const std::vector<std::vector<uint32_t>> &lists, const std::vector<uint32_t> &labels, const rk_group_rule &r)
{
    Result out;
    const uint32_t n = (uint32_t)labels.size();
    out.off.push_back(0);
    for (uint32_t l = 0; l < n; l++) {
        unsigned long long m = 0;
        for (uint32_t v = 0; v < n; v++) m += labels[v] == l;
        if (!m) continue;
        out.label.push_back(l);
        out.size.push_back((uint32_t)m);
        for (size_t u = 0; u < lists.size(); u++) {
            const std::set<uint32_t> who(lists[u].begin(), lists[u].end());
            unsigned long long c = 0;
            for (uint32_t v : who) c += labels[v] == l;
            if (c >= r.min_count && c * r.share_den >= (unsigned long long)r.share_num * m && (!r.only || c == who.size())) out.kept.push_back(u);
        }
        out.off.push_back(out.kept.size());
    }
    return out;
}

struct Call {
    uint64_t *off = (uint64_t *)0x10, *kept = (uint64_t *)0x10;
    uint32_t *label = (uint32_t *)0x10, *size = (uint32_t *)0x10, k = 77;
    bool untouched() const { return off == (uint64_t *)0x10 && kept == (uint64_t *)0x10 && label == (uint32_t *)0x10 && size == (uint32_t *)0x10 && k == 77; }
    void release()
    {
        rk_free_host(off);
        rk_free_host(kept);
        rk_free_host(label);
        rk_free_host(size);
    }
};

static int call(const std::vector<std::vector<uint32_t>> &lists, const std::vector<uint32_t> &labels, const rk_group_rule *r, Call *c)
{
    std::vector<uint32_t> postings, counts;
    for (const auto &l : lists) {
        postings.insert(postings.end(), l.begin(), l.end());
        counts.push_back((uint32_t)l.size());
    }
    return rk_group_lists(postings.data(), counts.data(), lists.size(), (uint32_t)labels.size(), labels.data(), r, &c->off, &c->kept, &c->label, &c->size, &c->k);
}

static Result taken(Call &c)
{
    Result r;
    r.off.assign(c.off, c.off + c.k + 1);
    if (r.off.back()) r.kept.assign(c.kept, c.kept + r.off.back());
    if (c.k) {
        r.label.assign(c.label, c.label + c.k);
        r.size.assign(c.size, c.size + c.k);
    }
    c.release();
    return r;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
    std::mt19937 rng(20261020);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    static const rk_group_rule named[4] = {{0, 1, 1, 0}, {1, 1, 1, 0}, {1, 2, 1, 0}, {0, 1, 1, 1}};
    unsigned long long kept = 0, empty_groups = 0, strangers = 0;
    for (int it = 0; it < 2000; it++) {
        const uint32_t n = 1 + below(12), n_lists = below(21);
        std::vector<uint32_t> labels(n);
        for (auto &l : labels) l = below(4) ? below(n) : kNone;
        std::vector<std::vector<uint32_t>> lists(n_lists);
        for (auto &l : lists) {
            l.resize(below(2 * n + 1));   // (an empty list may stand in the middle; repeats happen)
            for (auto &v : l) v = below(n);
        }
        rk_group_rule r = named[it % 4];
        if (it % 5 == 4) {
            r.share_den = 1 + below(4);
            r.share_num = below(r.share_den + 1);
            r.min_count = 1 + below(3);
            r.only = below(2);
        }
        Call c;
        CHECK(call(lists, labels, &r, &c) == RK_OK);
        const Result got = taken(c), want = plain(lists, labels, r);
        CHECK(got == want);
        kept += got.kept.size();
        for (size_t g = 0; g + 1 < got.off.size(); g++) empty_groups += got.off[g] == got.off[g + 1];
        for (uint32_t v = 0; v < n; v++) strangers += labels[v] != kNone && labels[labels[v]] != labels[v];
    }
    CHECK(kept > 5000 && empty_groups > 500 && strangers > 2000);
    {   // no group, no list, no genome
        Call c;
        CHECK(call({{0, 1}, {1}}, {kNone, kNone}, &named[0], &c) == RK_OK && c.k == 0 && c.off && c.off[0] == 0 && !c.kept && !c.label && !c.size);
        c.release();
        Call d;
        CHECK(rk_group_lists(nullptr, nullptr, 0, 2, std::vector<uint32_t>{1, 1}.data(), &named[1], &d.off, &d.kept, &d.label, &d.size, &d.k) == RK_OK);
        CHECK(d.k == 1 && d.off[0] == 0 && d.off[1] == 0 && !d.kept && d.label[0] == 1 && d.size[0] == 2);
        d.release();
        Call e;
        CHECK(rk_group_lists(nullptr, nullptr, 0, 0, nullptr, &named[0], &e.off, &e.kept, &e.label, &e.size, &e.k) == RK_OK && e.k == 0 && e.off[0] == 0);
        e.release();
    }
    {   // the refusals write nothing
        Call c;
        const std::vector<std::vector<uint32_t>> lists = {{0, 1}, {1}};
        CHECK(call({{0, 2}, {1}}, {0, kNone}, &named[0], &c) == RK_ERR_ARG);
        CHECK(call(lists, {0, 2}, &named[0], &c) == RK_ERR_ARG && call(lists, {0, kNone - 1}, &named[0], &c) == RK_ERR_ARG);
        static const rk_group_rule bad[4] = {{0, 0, 1, 0}, {2, 1, 1, 0}, {0, 1, 0, 0}, {0, 1, 1, 2}};
        for (const rk_group_rule &r : bad) CHECK(call(lists, {0, kNone}, &r, &c) == RK_ERR_ARG);
        CHECK(call(lists, {0, kNone}, nullptr, &c) == RK_ERR_ARG);
        const uint32_t p[3] = {0, 1, 1}, n2[2] = {2, 1}, lab[2] = {0, kNone};
        CHECK(rk_group_lists(nullptr, n2, 2, 2, lab, &named[0], &c.off, &c.kept, &c.label, &c.size, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, nullptr, 2, 2, lab, &named[0], &c.off, &c.kept, &c.label, &c.size, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, n2, 2, 2, nullptr, &named[0], &c.off, &c.kept, &c.label, &c.size, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, n2, 2, 2, lab, &named[0], nullptr, &c.kept, &c.label, &c.size, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, n2, 2, 2, lab, &named[0], &c.off, nullptr, &c.label, &c.size, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, n2, 2, 2, lab, &named[0], &c.off, &c.kept, nullptr, &c.size, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, n2, 2, 2, lab, &named[0], &c.off, &c.kept, &c.label, nullptr, &c.k) == RK_ERR_ARG);
        CHECK(rk_group_lists(p, n2, 2, 2, lab, &named[0], &c.off, &c.kept, &c.label, &c.size, nullptr) == RK_ERR_ARG);
        CHECK(c.untouched());
        CHECK(rk_group_sketches(nullptr, nullptr, lab, &named[0], nullptr, nullptr, nullptr, nullptr, nullptr) == RK_ERR_ARG);
    }
    printf("group_lists_check: 2000 collections, %llu kept (group, list) pairs, %llu empty groups: ok\n", kept, empty_groups);
    return 0;
}
