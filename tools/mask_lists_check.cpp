// Developer check: rk_mask_lists (host code of rk_mask.hip) against a plain restatement of the rule under the host sanitizers, as a
// stand-alone program -- 3,000 random small cases in both hash widths (0 .. 30 list hashes with counts 0 .. 5, 0 .. 6 queries of up to 40
// hashes in any order with repeats, some of them absent from the lists, every band with bounds in 0 .. 6 and UINT32_MAX), the cases
// without a query, a hash or a list, and the refusals (min_refs above max_refs, offsets that do not ascend from 0, list hashes that do
// not strictly ascend, null pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_mask.hip -x hip tools/mask_lists_check.cpp -o mask_lists_check && ./mask_lists_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>
#include "rk_internal.h"
// what rk_mask.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
int rk_index_ensure_dir(rk_ctx *, rk_index *, hipStream_t) { return -1; }
extern "C" int rk_index_export_lists(const rk_index *, uint32_t *, uint32_t *, uint32_t *) { return -1; }
extern "C" int rk_index_export64(const rk_index *, uint32_t *, uint64_t *, uint32_t *) { return -1; }
extern "C" int rk_sketches_download(const rk_sketches *, uint32_t *, uint64_t *) { return -1; }
extern "C" int rk_sketches_download64(const rk_sketches *, uint64_t *, uint64_t *) { return -1; }
extern "C" int rk_sketches_from_host(rk_ctx *, const uint32_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" int rk_sketches_from_host64(rk_ctx *, const uint64_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" int rk_sketches_download_counts(const rk_sketches *, uint32_t *) { return -1; }
extern "C" int rk_sketches_from_host_counts(rk_ctx *, const void *, int, const uint32_t *, const uint64_t *, uint32_t, rk_sketches **) { return -1; }
extern "C" void rk_sketches_free(rk_sketches *) {}
extern "C" void rk_free_host(void *p) { free(p); }

static const uint64_t kMark = 0x5A5A5A5A5A5A5A5AULL;
static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);     \
            failures++;                                                    \
        }                                                                  \
    } while (0)

template <class Hash> struct Case {
    std::vector<Hash> q, lists;
    std::vector<uint64_t> q_off;
    std::vector<uint32_t> counts;
};

// the rule, plainly: a map from hash to count, the queries walked in their order
template <class Hash> static void plain(const Case<Hash> &c, const rk_mask_rule &r, std::vector<Hash> *kept, std::vector<uint64_t> *off, rk_mask_stats *st)
{
    std::map<Hash, uint32_t> held;
    for (size_t u = 0; u < c.lists.size(); u++) held[c.lists[u]] = c.counts[u];
    memset(st, 0, sizeof *st);
    off->assign(1, 0);
    for (size_t i = 0; i + 1 < c.q_off.size(); i++) {
        for (uint64_t j = c.q_off[i]; j < c.q_off[i + 1]; j++) {
            const auto it = held.find(c.q[j]);
            const uint32_t n = it == held.end() ? 0u : it->second;
            st->matched += n > 0;
            if (r.min_refs <= n && n <= r.max_refs) kept->push_back(c.q[j]);
        }
        off->push_back(kept->size());
        st->emptied += c.q_off[i + 1] > c.q_off[i] && (*off)[i + 1] == (*off)[i];
    }
    st->hashes = c.q_off.back();
    st->kept = kept->size();
}

template <class Hash> static void run_case(const Case<Hash> &c, const rk_mask_rule &r)
{
    const uint32_t nq = (uint32_t)c.q_off.size() - 1;
    std::vector<Hash> want;
    std::vector<uint64_t> want_off, off((size_t)nq + 1, kMark);
    rk_mask_stats want_st, st;
    plain(c, r, &want, &want_off, &want_st);
    void *h = (void *)(uintptr_t)kMark;
    const int rc = rk_mask_lists(c.q.empty() ? nullptr : c.q.data(), sizeof(Hash) == 8, c.q_off.data(), nq, c.lists.empty() ? nullptr : c.lists.data(),
                                 c.counts.empty() ? nullptr : c.counts.data(), c.lists.size(), &r, &h, off.data(), &st);
    CHECK(rc == RK_OK);
    if (rc != RK_OK) return;
    CHECK(off == want_off);
    CHECK((h == nullptr) == want.empty());
    CHECK(want.empty() || !memcmp(h, want.data(), want.size() * sizeof(Hash)));
    CHECK(st.hashes == want_st.hashes && st.kept == want_st.kept && st.matched == want_st.matched && st.emptied == want_st.emptied && st.path == 2);
    CHECK(st.tile_hashes && st.tiles == (st.hashes + st.tile_hashes - 1) / st.tile_hashes);
    rk_free_host(h);
}

template <class Hash> static void random_cases(std::mt19937_64 &rng, int n_cases)
{
    const uint32_t bounds[] = {0, 1, 2, 3, 4, 5, 6, 0xFFFFFFFFu};
    for (int k = 0; k < n_cases; k++) {
        Case<Hash> c;
        const Hash top = sizeof(Hash) == 8 ? (Hash)0xFFFFFFFFFFFFFFFFULL : (Hash)0xFFFFFFFFu;
        std::vector<Hash> universe;
        for (int i = 0, n = (int)(rng() % 45) + 1; i < n; i++) universe.push_back(rng() % 8 == 0 ? top - (Hash)(rng() % 4) : (Hash)(rng() % 200));
        for (int i = 0, n = (int)(rng() % 31); i < n; i++) c.lists.push_back(universe[rng() % universe.size()]);
        std::sort(c.lists.begin(), c.lists.end());
        c.lists.erase(std::unique(c.lists.begin(), c.lists.end()), c.lists.end());
        for (size_t u = 0; u < c.lists.size(); u++) c.counts.push_back((uint32_t)(rng() % 6));
        c.q_off.push_back(0);
        for (int i = 0, n = (int)(rng() % 7); i < n; i++) {
            for (int j = 0, m = (int)(rng() % 41) * (int)(rng() % 3 != 0); j < m; j++) c.q.push_back(universe[rng() % universe.size()]);
            c.q_off.push_back(c.q.size());
        }
        for (int b = 0; b < 4; b++) {
            rk_mask_rule r{bounds[rng() % 8], bounds[rng() % 8]};
            if (r.min_refs > r.max_refs) std::swap(r.min_refs, r.max_refs);
            run_case(c, r);
        }
        run_case(c, rk_mask_rule{0, 0});
        run_case(c, rk_mask_rule{1, 0xFFFFFFFFu});
    }
}

template <class Hash> static void refusals()
{
    const Hash q[3] = {5, 3, 9}, lists[2] = {3, 9}, flat[2] = {9, 9}, down[2] = {9, 3};
    const uint64_t q_off[3] = {0, 2, 3}, late[3] = {1, 2, 3}, back[3] = {0, 2, 1};
    const uint32_t counts[2] = {1, 2};
    const rk_mask_rule ok{0, 0}, bad{2, 1};
    const int wide = sizeof(Hash) == 8;
    void *h = (void *)(uintptr_t)kMark;
    uint64_t off[3] = {kMark, kMark, kMark};
    rk_mask_stats st;
    memset(&st, 0x5A, sizeof st);
    CHECK(rk_mask_lists(q, wide, q_off, 2, lists, counts, 2, &bad, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, late, 2, lists, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, back, 2, lists, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, flat, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, down, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(nullptr, wide, q_off, 2, lists, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, nullptr, 2, lists, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, nullptr, counts, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, lists, nullptr, 2, &ok, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, lists, counts, 2, nullptr, &h, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, lists, counts, 2, &ok, nullptr, off, &st) == RK_ERR_ARG);
    CHECK(rk_mask_lists(q, wide, q_off, 2, lists, counts, 2, &ok, &h, nullptr, &st) == RK_ERR_ARG);
    CHECK(h == (void *)(uintptr_t)kMark && off[0] == kMark && off[1] == kMark && off[2] == kMark && st.hashes == kMark && st.pad_ == 0x5A5A5A5Au);
    // the good call writes, with and without stats
    CHECK(rk_mask_lists(q, wide, q_off, 2, lists, counts, 2, &ok, &h, off, nullptr) == RK_OK);
    CHECK(off[0] == 0 && off[1] == 1 && off[2] == 1 && h && ((const Hash *)h)[0] == 5);
    rk_free_host(h);
    // no query; queries without hashes; no list
    uint64_t zero[1] = {0}, one[1] = {kMark};
    CHECK(rk_mask_lists(nullptr, wide, zero, 0, lists, counts, 2, &ok, &h, one, &st) == RK_OK && h == nullptr && one[0] == 0 && st.hashes == 0 && st.tiles == 0);
    const uint64_t empties[3] = {0, 0, 0};
    CHECK(rk_mask_lists(nullptr, wide, empties, 2, nullptr, nullptr, 0, &ok, &h, off, &st) == RK_OK && h == nullptr && off[2] == 0 && st.emptied == 0);
    CHECK(rk_mask_lists(q, wide, q_off, 2, nullptr, nullptr, 0, &ok, &h, off, &st) == RK_OK && off[2] == 3 && st.kept == 3 && st.matched == 0);
    rk_free_host(h);
}

int main()
{
    std::mt19937_64 rng(20261021);
    random_cases<uint32_t>(rng, 1500);
    random_cases<uint64_t>(rng, 1500);
    refusals<uint32_t>();
    refusals<uint64_t>();
    if (failures) {
        fprintf(stderr, "mask_lists_check: %d check(s) FAILED\n", failures);
        return 1;
    }
    printf("mask_lists_check: ok (3000 random cases in two widths, the empty cases and the refusals)\n");
    return 0;
}
