// Developer check: rk_lca_lists and rk_lca_call (host code of rk_lca.hip) against a plain restatement of the rule under the host
// sanitizers, as a stand-alone program -- 3,000 random small cases (taxonomies of 1 .. 12 nodes in random numbering, 0 .. 8 references of
// which some are unlabelled, 0 .. 25 lists of 0 .. 6 postings with repeats, 0 .. 6 queries of up to 30 matched elements, every row shard of
// 1 .. 3), on each tally the call under 8 rules, a path of 300,000 nodes, the empty cases and the refusals (sums beyond 32 bits among
// them), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_lca.hip -x hip tools/lca_lists_check.cpp -o lca_lists_check && ./lca_lists_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>
#include "rk_internal.h"
// what rk_lca.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
int rk_read_back(rk_ctx *, void *, const void *, size_t, hipStream_t) { return -1; }
int rk_index_ensure_dir(rk_ctx *, rk_index *, hipStream_t) { return -1; }
int rk_prim_sort_pairs_u64_u32(rk_ctx *, const uint64_t *, uint64_t *, const uint32_t *, uint32_t *, uint64_t, unsigned, hipStream_t) { return -1; }
int rk_prim_inclusive_scan_u32(rk_ctx *, const uint32_t *, uint32_t *, uint64_t, hipStream_t) { return -1; }
extern "C" int rk_index_export_lists(const rk_index *, uint32_t *, uint32_t *, uint32_t *) { return -1; }
extern "C" int rk_index_export64(const rk_index *, uint32_t *, uint64_t *, uint32_t *) { return -1; }
extern "C" int rk_sketches_download(const rk_sketches *, uint32_t *, uint64_t *) { return -1; }
extern "C" int rk_sketches_download64(const rk_sketches *, uint64_t *, uint64_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

static const uint64_t kMark = 0x5A5A5A5A5A5A5A5AULL;
static const uint32_t kMark32 = 0x5A5A5A5Au, kNone = RK_LCA_NONE;
static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);     \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// the taxonomy, plainly: the nodes from t up to the root
static std::vector<uint32_t> root_path(const std::vector<uint32_t> &parent, uint32_t t)
{
    std::vector<uint32_t> p{t};
    while (parent[p.back()] != p.back()) p.push_back(parent[p.back()]);
    return p;
}
static bool above(const std::vector<uint32_t> &parent, uint32_t a, uint32_t t)   // a is t or an ancestor of t
{
    const std::vector<uint32_t> p = root_path(parent, t);
    return std::find(p.begin(), p.end(), a) != p.end();
}
// the LCA of a non-empty set: the first node of one member's root path that is above all of them
static uint32_t plain_lca(const std::vector<uint32_t> &parent, const std::vector<uint32_t> &nodes)
{
    for (const uint32_t a : root_path(parent, nodes[0])) {
        bool all = true;
        for (const uint32_t t : nodes) all = all && above(parent, a, t);
        if (all) return a;
    }
    return kNone;
}

struct Case {
    std::vector<uint32_t> parent, taxa, postings, counts;
    std::vector<uint64_t> q_off, q_lists;
};

static void run_case(const Case &c, const rk_lca_opts &o)
{
    const uint32_t nq = (uint32_t)c.q_off.size() - 1;
    // per list its lca; per selected query a map taxon -> direct
    std::vector<uint32_t> list_lca;
    for (size_t u = 0, pos = 0; u < c.counts.size(); pos += c.counts[u++]) {
        std::vector<uint32_t> nodes;
        for (size_t k = pos; k < pos + c.counts[u]; k++)
            if (c.taxa[c.postings[k]] != kNone) nodes.push_back(c.taxa[c.postings[k]]);
        list_lca.push_back(nodes.empty() ? kNone : plain_lca(c.parent, nodes));
    }
    const uint32_t rb = o.row_block ? o.row_block : 1, rs = o.row_step ? o.row_step : 1;
    std::vector<rk_lca_count> want;
    std::vector<uint64_t> want_off{0};
    std::vector<uint32_t> want_matched(nq, kMark32), want_unl(nq, kMark32);
    for (uint32_t q = 0; q < nq; q++) {
        if (q / rb >= o.row_first && (q / rb - o.row_first) % rs == 0) {
            std::map<uint32_t, uint32_t> direct;
            want_matched[q] = (uint32_t)(c.q_off[q + 1] - c.q_off[q]);
            want_unl[q] = 0;
            for (uint64_t j = c.q_off[q]; j < c.q_off[q + 1]; j++) {
                if (list_lca[c.q_lists[j]] == kNone) want_unl[q]++;
                else direct[list_lca[c.q_lists[j]]]++;
            }
            for (const auto &kv : direct) want.push_back(rk_lca_count{kv.first, kv.second});
        }
        want_off.push_back(want.size());
    }
    std::vector<uint64_t> off((size_t)nq + 1, kMark);
    std::vector<uint32_t> matched(nq, kMark32), unl(nq, kMark32);
    rk_lca_count *recs = (rk_lca_count *)(uintptr_t)kMark;
    uint64_t n = kMark;
    rk_lca_stats st;
    const int rc = rk_lca_lists(c.postings.empty() ? nullptr : c.postings.data(), c.counts.empty() ? nullptr : c.counts.data(), c.counts.size(), c.q_off.data(),
                                c.q_lists.empty() ? nullptr : c.q_lists.data(), nq, (uint32_t)c.taxa.size(), c.taxa.empty() ? nullptr : c.taxa.data(),
                                c.parent.data(), (uint32_t)c.parent.size(), &o, off.data(), &recs, &n, nq ? matched.data() : nullptr, nq ? unl.data() : nullptr, &st);
    CHECK(rc == RK_OK);
    if (rc != RK_OK) return;
    CHECK(off == want_off && n == want.size() && (recs == nullptr) == want.empty());
    CHECK(want.empty() || !memcmp(recs, want.data(), want.size() * sizeof(rk_lca_count)));
    CHECK(matched == want_matched && unl == want_unl);   // (the entries of unselected rows keep their mark)
    CHECK(st.path == 2 && st.records == want.size() && st.lists == c.counts.size() && st.postings == c.postings.size());
    // the call on these tallies, against the definition: clade and score by scanning every node
    const rk_lca_rule rules[] = {{1, 0, 1, 0}, {1, 1, 1, 0}, {2, 1, 1, 0}, {1, 1, 2, 0}, {1, 2, 3, 1}, {2, 1, 3, 1}, {1, 1, 1, 1}, {3, 0, 1, 1}};
    const uint32_t T = (uint32_t)c.parent.size();
    std::vector<uint32_t> sizes;
    for (uint32_t q = 0; q < nq; q++) sizes.push_back((uint32_t)(c.q_off[q + 1] - c.q_off[q]) + q % 3);
    for (const rk_lca_rule &r : rules) {
        std::vector<rk_lca_called> called(nq);
        std::vector<uint32_t> clade_out(want.size(), kMark32);
        CHECK(rk_lca_call(recs, off.data(), nq, sizes.data(), c.parent.data(), T, &r, nq ? called.data() : nullptr, clade_out.data()) == RK_OK);
        for (uint32_t q = 0; q < nq; q++) {
            std::vector<uint64_t> clade(T, 0), score(T, 0);
            uint64_t retained = 0, best = 0;
            uint32_t kept = 0, root = 0;
            for (uint32_t a = 0; a < T; a++) {
                if (c.parent[a] == a) root = a;
                for (uint64_t j = off[q]; j < off[q + 1]; j++)
                    if (want[j].direct >= r.min_count) {
                        if (above(c.parent, a, want[j].taxon)) clade[a] += want[j].direct;
                        if (above(c.parent, want[j].taxon, a)) score[a] += want[j].direct;
                    }
            }
            std::vector<uint32_t> top;
            for (uint64_t j = off[q]; j < off[q + 1]; j++)
                if (want[j].direct >= r.min_count) {
                    retained += want[j].direct;
                    kept++;
                    best = std::max(best, score[want[j].taxon]);
                }
            for (uint64_t j = off[q]; j < off[q + 1]; j++)
                if (want[j].direct >= r.min_count && score[want[j].taxon] == best) top.push_back(want[j].taxon);
            rk_lca_called w = {kNone, kNone, 0, 0, (uint32_t)retained, kept};
            if (kept) {
                w.candidate = plain_lca(c.parent, top);
                w.score = (uint32_t)best;
                w.clade = (uint32_t)clade[root];
                const uint64_t D = r.denom ? sizes[q] : retained;
                for (const uint32_t a : root_path(c.parent, w.candidate))
                    if (clade[a] * r.conf_den >= (uint64_t)r.conf_num * D) {
                        w.taxon = a;
                        w.clade = (uint32_t)clade[a];
                        break;
                    }
            }
            CHECK(!memcmp(&w, &called[q], sizeof w));
            for (uint64_t j = off[q]; j < off[q + 1]; j++) CHECK(clade_out[j] == clade[want[j].taxon]);
        }
    }
    rk_free_host(recs);
}

static void random_cases(std::mt19937_64 &rng, int n_cases)
{
    for (int k = 0; k < n_cases; k++) {
        Case c;
        const uint32_t T = (uint32_t)(rng() % 12) + 1, N = (uint32_t)(rng() % 9);
        std::vector<uint32_t> order(T);
        for (uint32_t t = 0; t < T; t++) order[t] = t;
        std::shuffle(order.begin(), order.end(), rng);
        c.parent.assign(T, 0);
        for (uint32_t i = 0; i < T; i++) c.parent[order[i]] = i ? order[rng() % i] : order[0];
        for (uint32_t v = 0; v < N; v++) c.taxa.push_back(rng() % 5 == 0 ? kNone : (uint32_t)(rng() % T));
        const int n_lists = N ? (int)(rng() % 26) : 0;
        for (int u = 0; u < n_lists; u++) {
            c.counts.push_back((uint32_t)(rng() % 7));
            for (uint32_t j = 0; j < c.counts.back(); j++) c.postings.push_back((uint32_t)(rng() % N));
        }
        c.q_off.push_back(0);
        for (int i = 0, n = (int)(rng() % 7); i < n; i++) {
            std::vector<uint64_t> mine;
            for (int j = 0, m = n_lists ? (int)(rng() % 31) * (int)(rng() % 3 != 0) : 0; j < m; j++) mine.push_back(rng() % n_lists);
            std::sort(mine.begin(), mine.end());
            c.q_lists.insert(c.q_lists.end(), mine.begin(), mine.end());
            c.q_off.push_back(c.q_lists.size());
        }
        run_case(c, rk_lca_opts{0, 0, 0});
        const uint32_t step = (uint32_t)(rng() % 3) + 1;
        for (uint32_t first = 0; first < step; first++) run_case(c, rk_lca_opts{first, step, (uint32_t)(rng() % 3)});
    }
}

static void long_path()
{
    // a path of 300,000 nodes, 7 (the root) <- 8 <- .. <- T - 1 <- 0 <- 1 <- .. <- 6: nothing recurses.  List 0 is held by references in
    // 6 and T / 2 and an unlabelled one (its lca is T / 2), list 1 by 6 and the unlabelled one.  Worked by hand: the plain restatement
    // above costs T per ancestor test.
    const uint32_t T = 300000;
    std::vector<uint32_t> parent(T);
    for (uint32_t t = 0; t < T; t++) parent[t] = t == 7 ? 7 : t == 0 ? T - 1 : t - 1;
    const uint32_t taxa[3] = {6, T / 2, kNone}, postings[5] = {0, 1, 2, 0, 2}, counts[2] = {3, 2};
    const uint64_t q_off[2] = {0, 3}, ql[3] = {0, 0, 1};
    const rk_lca_opts o{0, 0, 0};
    uint64_t off[2], n = 0;
    uint32_t matched = 0, unl = 0, clade[2];
    rk_lca_count *recs = nullptr;
    CHECK(rk_lca_lists(postings, counts, 2, q_off, ql, 1, 3, taxa, parent.data(), T, &o, off, &recs, &n, &matched, &unl, nullptr) == RK_OK);
    CHECK(n == 2 && off[1] == 2 && matched == 3 && unl == 0 && recs && recs[0].taxon == 6 && recs[0].direct == 1 && recs[1].taxon == T / 2 && recs[1].direct == 2);
    if (n != 2) return;
    rk_lca_called c;
    const rk_lca_rule kraken{1, 0, 1, 0}, all{1, 1, 1, 0};
    CHECK(rk_lca_call(recs, off, 1, nullptr, parent.data(), T, &kraken, &c, clade) == RK_OK);
    CHECK(c.taxon == 6 && c.candidate == 6 && c.clade == 1 && c.score == 3 && c.retained == 3 && c.n_taxa == 2 && clade[0] == 1 && clade[1] == 3);
    CHECK(rk_lca_call(recs, off, 1, nullptr, parent.data(), T, &all, &c, nullptr) == RK_OK && c.taxon == T / 2 && c.candidate == 6 && c.clade == 3);
    rk_free_host(recs);
}

static void refusals()
{
    const uint32_t postings[3] = {0, 1, 1}, counts[2] = {2, 1}, taxa[2] = {1, kNone}, parent[2] = {0, 0}, bad_post[3] = {0, 2, 1}, bad_taxa[2] = {2, kNone};
    const uint32_t two_roots[2] = {0, 1}, no_root[2] = {1, 0}, beyond[2] = {0, 2}, cycle[3] = {0, 2, 1};
    const uint64_t q_off[3] = {0, 2, 3}, ql[3] = {0, 0, 1}, late[3] = {1, 2, 3}, back[3] = {0, 3, 2}, far[3] = {0, 2, 1}, down[3] = {1, 0, 1};
    const rk_lca_opts o{0, 0, 0};
    uint64_t off[3] = {kMark, kMark, kMark}, n = kMark;
    uint32_t matched[2] = {kMark32, kMark32}, unl[2] = {kMark32, kMark32};
    rk_lca_count *recs = (rk_lca_count *)(uintptr_t)kMark;
    rk_lca_stats st;
    memset(&st, 0x5A, sizeof st);
#define LISTS(P, C, QO, QL, NREF, TX, PAR, T, O, OFF, R, N, M, U) rk_lca_lists(P, C, 2, QO, QL, 2, NREF, TX, PAR, T, O, OFF, R, N, M, U, &st)
    CHECK(LISTS(nullptr, counts, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, nullptr, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, nullptr, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, nullptr, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, nullptr, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, nullptr, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, nullptr, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, &o, nullptr, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, &o, off, nullptr, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, nullptr, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, &n, nullptr, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, nullptr) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 0, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, two_roots, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, no_root, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, beyond, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, cycle, 3, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 2, bad_taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, late, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, back, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, far, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, down, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(bad_post, counts, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_ARG);
    CHECK(LISTS(postings, counts, q_off, ql, 0x80000000u, nullptr, parent, 2, &o, off, &recs, &n, matched, unl) == RK_ERR_UNSUPPORTED);
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 0x80000000u, &o, off, &recs, &n, matched, unl) == RK_ERR_UNSUPPORTED);
    CHECK(recs == (rk_lca_count *)(uintptr_t)kMark && n == kMark && off[0] == kMark && off[2] == kMark && matched[0] == kMark32 && unl[1] == kMark32 &&
          st.lists == kMark && st.threads == kMark32);
    // the good call writes: list 0 is held by reference 0 (node 1) and 1 (unlabelled), list 1 by 1 alone
    CHECK(LISTS(postings, counts, q_off, ql, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl) == RK_OK);
    CHECK(off[0] == 0 && off[1] == 1 && off[2] == 1 && n == 1 && recs && recs[0].taxon == 1 && recs[0].direct == 2 && matched[0] == 2 && matched[1] == 1 &&
          unl[0] == 0 && unl[1] == 1 && st.path == 2 && st.matched == 3 && st.unlabelled == 1);
    // rk_lca_call: bad rules, null pointers, a record beyond the nodes; nothing is written
    rk_lca_called called[2];
    memset(called, 0x5A, sizeof called);
    const uint32_t sizes[2] = {5, 5};
    const rk_lca_rule ok{1, 0, 1, 0}, r0{0, 0, 1, 0}, r1{1, 0, 0, 0}, r2{1, 2, 1, 0}, r3{1, 0, 1, 2}, sized{1, 1, 2, 1};
    const rk_lca_count twice[2] = {{1, 2}, {1, 1}}, outside[1] = {{2, 1}};
    const uint64_t two[2] = {0, 2}, one[2] = {0, 1};
    for (const rk_lca_rule *r : {&r0, &r1, &r2, &r3}) CHECK(rk_lca_call(recs, off, 2, sizes, parent, 2, r, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(recs, off, 2, nullptr, parent, 2, &sized, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(nullptr, off, 2, sizes, parent, 2, &ok, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(recs, nullptr, 2, sizes, parent, 2, &ok, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(recs, off, 2, sizes, nullptr, 2, &ok, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(recs, off, 2, sizes, parent, 2, nullptr, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(recs, off, 2, sizes, parent, 2, &ok, nullptr, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(recs, off, 2, sizes, two_roots, 2, &ok, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(twice, two, 1, sizes, parent, 2, &ok, called, nullptr) == RK_ERR_ARG);
    CHECK(rk_lca_call(outside, one, 1, sizes, parent, 2, &ok, called, nullptr) == RK_ERR_ARG);
    const rk_lca_count wide[2] = {{0, 0xFFFFFFFFu}, {1, 1}}, fits[2] = {{0, 0xFFFFFFFEu}, {1, 1}};   // sums of 2^32 and of 2^32 - 1
    CHECK(rk_lca_call(wide, two, 1, sizes, parent, 2, &ok, called, nullptr) == RK_ERR_UNSUPPORTED);
    CHECK(called[0].taxon == kMark32 && called[1].n_taxa == kMark32);
    CHECK(rk_lca_call(fits, two, 1, sizes, parent, 2, &ok, called, nullptr) == RK_OK && called[0].taxon == 1 && called[0].score == 0xFFFFFFFFu &&
          called[0].retained == 0xFFFFFFFFu && called[0].clade == 1);
    memset(called, 0x5A, sizeof called);
    CHECK(rk_lca_call(recs, off, 2, nullptr, parent, 2, &ok, called, nullptr) == RK_OK && called[0].taxon == 1 && called[0].retained == 2 &&
          called[1].taxon == kNone && called[1].n_taxa == 0);
    rk_free_host(recs);
    // no query; no list; no reference
    uint64_t zero[1] = {0}, out0[1] = {kMark};
    CHECK(rk_lca_lists(nullptr, nullptr, 0, zero, nullptr, 0, 0, nullptr, parent, 2, &o, out0, &recs, &n, nullptr, nullptr, &st) == RK_OK && out0[0] == 0 &&
          recs == nullptr && n == 0 && st.rows == 0);
    const uint64_t empties[3] = {0, 0, 0};
    CHECK(rk_lca_lists(nullptr, nullptr, 0, empties, nullptr, 2, 2, taxa, parent, 2, &o, off, &recs, &n, matched, unl, nullptr) == RK_OK && off[2] == 0 &&
          matched[0] == 0 && unl[1] == 0 && recs == nullptr);
    CHECK(rk_lca_call(nullptr, zero, 0, nullptr, parent, 2, &ok, nullptr, nullptr) == RK_OK);
#undef LISTS
}

int main()
{
    std::mt19937_64 rng(20261021);
    random_cases(rng, 3000);
    long_path();
    refusals();
    if (failures) {
        fprintf(stderr, "lca_lists_check: %d check(s) FAILED\n", failures);
        return 1;
    }
    printf("lca_lists_check: ok (3000 random cases under every row shard and 8 rules, a path of 300,000 nodes, the empty cases and the refusals)\n");
    return 0;
}
