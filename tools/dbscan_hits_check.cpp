// Developer check: rk_dbscan_hits (host code of rk_dbscan.hip) against a plain restatement of the rule under the host sanitizers, as a
// stand-alone program -- 600 random small graphs (n = 1 .. 24, both metrics, min_pts = 1 .. n + 2, equal ratios from different counts),
// each also in shuffled record order with rows and cols swapped, without the optional outputs, and the refusals (a genome >= n, row ==
// col, min_pts == 0, null pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_dbscan.hip -x hip tools/dbscan_hits_check.cpp -o dbscan_hits_check && ./dbscan_hits_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "rk_internal.h"
// what rk_dbscan.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
void *rk_pinned_scratch(rk_ctx *, size_t) { return nullptr; }
uint64_t rk_host_exact_distances(rk_hit *, uint64_t, const rk_dist_opts *) { return 0; }
extern "C" int rk_dist_rows_dev(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit *, uint64_t, uint64_t *, void *) { return -1; }
extern "C" int rk_dist_rows(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit **, uint64_t *, int32_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

static const int kTriples[5][3] = {{20, 50, 50}, {40, 60, 60}, {60, 70, 70}, {20, 40, 40}, {25, 50, 50}};   // 20/60 ties 25/75
static const uint32_t kNone = RK_DBSCAN_NOISE;

struct Out {
    std::vector<uint32_t> label, via, deg;
    std::vector<uint8_t> kind;
    explicit Out(uint32_t n) : label(n, 77), via(n, 77), deg(n, 77), kind(n, 77) {}
    bool operator==(const Out &o) const { return label == o.label && via == o.via && deg == o.deg && kind == o.kind; }
};

// record a (of neighbour xa) before record b (of neighbour xb): integers only
static bool before(const rk_hit &a, uint32_t xa, const rk_hit &b, uint32_t xb, int metric)
{
    const long long ca = a.common, cb = b.common;
    const long long ua = metric ? std::min(a.size0, a.size1) : a.size0 + a.size1 - a.common, ub = metric ? std::min(b.size0, b.size1) : b.size0 + b.size1 - b.common;
    if (ca * ub != cb * ua) return ca * ub > cb * ua;
    return xa < xb;
}

// the rule, plainly: an adjacency matrix, labels by repeated relaxation over the core-core edges
static Out plain(const std::vector<rk_hit> &hits, uint32_t n, uint32_t min_pts, int metric)
{
    Out o(n);
    std::vector<int> edge((size_t)n * n, -1);
    for (size_t e = 0; e < hits.size(); e++) edge[(size_t)hits[e].row * n + hits[e].col] = edge[(size_t)hits[e].col * n + hits[e].row] = (int)e;
    for (uint32_t v = 0; v < n; v++) {
        o.deg[v] = 0;
        for (uint32_t x = 0; x < n; x++) o.deg[v] += edge[(size_t)v * n + x] >= 0;
        o.kind[v] = (uint64_t)o.deg[v] + 1 >= min_pts ? 2 : 0;
        o.label[v] = o.kind[v] ? v : kNone;
        o.via[v] = kNone;
    }
    for (bool changed = true; changed;) {
        changed = false;
        for (const rk_hit &h : hits)
            if (o.kind[h.row] == 2 && o.kind[h.col] == 2 && o.label[h.row] != o.label[h.col]) {
                o.label[h.row] = o.label[h.col] = std::min(o.label[h.row], o.label[h.col]);
                changed = true;
            }
    }
    for (uint32_t v = 0; v < n; v++) {
        if (o.kind[v]) continue;
        for (uint32_t x = 0; x < n; x++) {
            const int e = edge[(size_t)v * n + x];
            if (e < 0 || o.kind[x] != 2) continue;
            if (o.via[v] == kNone || before(hits[(size_t)e], x, hits[(size_t)edge[(size_t)v * n + o.via[v]]], o.via[v], metric)) o.via[v] = x;
        }
        if (o.via[v] != kNone) {
            o.kind[v] = 1;
            o.label[v] = o.label[o.via[v]];
        }
    }
    return o;
}

static int call(const std::vector<rk_hit> &hits, uint32_t n, uint32_t min_pts, int metric, Out *o, bool all = true)
{
    return rk_dbscan_hits(hits.empty() ? nullptr : hits.data(), hits.size(), n, min_pts, metric, o->label.data(), o->kind.data(), all ? o->via.data() : nullptr,
                          all ? o->deg.data() : nullptr);
}

int main()
{
    std::mt19937 rng(29);
    unsigned long borders = 0;
    for (int c = 0; c < 600; c++) {
        const uint32_t n = 1 + c % 24, min_pts = 1 + rng() % (n + 2);
        const int metric = c & 1;
        std::vector<rk_hit> hits;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++)
                if (rng() % (2 + c % 5) == 0) {
                    const int *t = kTriples[rng() % 5];
                    hits.push_back(rk_hit{i, j, t[0], t[1], t[2], 0, 0.25 + (double)hits.size(), 0.5 + (double)hits.size()});
                }
        const Out want = plain(hits, n, min_pts, metric);
        borders += (unsigned long)std::count(want.kind.begin(), want.kind.end(), (uint8_t)1);
        Out got(n);
        if (call(hits, n, min_pts, metric, &got) != RK_OK || !(got == want)) { printf("rk_dbscan_hits: mismatch at case %d\n", c); return 1; }
        std::vector<rk_hit> other = hits;   // shuffled, rows and cols swapped: sizes travel with their genome
        std::shuffle(other.begin(), other.end(), rng);
        for (rk_hit &h : other) {
            std::swap(h.row, h.col);
            std::swap(h.size0, h.size1);
        }
        Out again(n);
        if (call(other, n, min_pts, metric, &again) != RK_OK || !(again == want)) { printf("rk_dbscan_hits: record order matters at case %d\n", c); return 1; }
        Out two(n);   // without the optional outputs
        if (call(hits, n, min_pts, metric, &two, false) != RK_OK || two.label != want.label || two.kind != want.kind || two.via != Out(n).via || two.deg != Out(n).deg) {
            printf("rk_dbscan_hits: optional outputs at case %d\n", c);
            return 1;
        }
        // refusals: nothing is written
        const Out clean(n);
        Out r(n);
        rk_hit bad[3] = {{0, n, 25, 50, 50, 0, 0, 0}, {n + 5, 0, 25, 50, 50, 0, 0, 0}, {n - 1, n - 1, 25, 50, 50, 0, 0, 0}};
        for (const rk_hit &b : bad) {
            std::vector<rk_hit> h2 = hits;
            h2.insert(h2.begin() + (long)(rng() % (h2.size() + 1)), b);
            if (call(h2, n, min_pts, metric, &r) != RK_ERR_ARG || !(r == clean)) { printf("rk_dbscan_hits: bad record accepted or something written at case %d\n", c); return 1; }
        }
        if (call(hits, n, 0, metric, &r) != RK_ERR_ARG || !(r == clean)) { printf("rk_dbscan_hits: min_pts 0 accepted at case %d\n", c); return 1; }
        if (rk_dbscan_hits(hits.data(), hits.size(), n, min_pts, metric, nullptr, r.kind.data(), r.via.data(), r.deg.data()) != RK_ERR_ARG ||
            rk_dbscan_hits(hits.data(), hits.size(), n, min_pts, metric, r.label.data(), nullptr, r.via.data(), r.deg.data()) != RK_ERR_ARG ||
            rk_dbscan_hits(nullptr, hits.size() + 1, n, min_pts, metric, r.label.data(), r.kind.data(), r.via.data(), r.deg.data()) != RK_ERR_ARG || !(r == clean)) {
            printf("rk_dbscan_hits: a null pointer accepted or something written at case %d\n", c);
            return 1;
        }
    }
    if (borders < 500) { printf("only %lu border genomes: the cases are too easy\n", borders); return 1; }
    if (rk_dbscan_hits(nullptr, 0, 0, 1, 0, nullptr, nullptr, nullptr, nullptr) != RK_OK) return 1;   // no genome: nothing to write
    if (rk_dbscan_rows(nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr) != RK_ERR_ARG) return 1;
    printf("rk_dbscan_hits: 600 cases clean (%lu border genomes)\n", borders);
    return 0;
}
