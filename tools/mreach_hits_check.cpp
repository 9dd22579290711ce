// Developer check: rk_mreach_hits and rk_mreach_cut (host code of rk_mreach.hip) against a plain restatement of the rule under the host
// sanitizers, as a stand-alone program -- 600 random small graphs (n = 1 .. 24, both metrics, min_pts = 1 .. n + 2, equal ratios from
// different counts), each also in shuffled record order with rows and cols swapped, without the optional output, cut at every distance
// that occurs, and the refusals (a genome >= n, row == col, min_pts == 0, null pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_mreach.hip -x hip tools/mreach_hits_check.cpp -o mreach_hits_check && ./mreach_hits_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "rk_internal.h"
// what rk_mreach.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
void *rk_pinned_scratch(rk_ctx *, size_t) { return nullptr; }
int rk_read_back(rk_ctx *, void *, const void *, size_t, hipStream_t) { return -1; }
int rk_prim_exclusive_scan_u32(rk_ctx *, const uint32_t *, uint32_t *, uint64_t, hipStream_t) { return -1; }
int rk_prim_sort_hits(rk_ctx *, const unsigned long long *, unsigned long long *, const rk_hit *, rk_hit *, uint64_t, unsigned, hipStream_t) { return -1; }
uint64_t rk_host_exact_distances(rk_hit *, uint64_t, const rk_dist_opts *) { return 0; }
extern "C" int rk_dist_rows_dev(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit *, uint64_t, uint64_t *, void *) { return -1; }
extern "C" int rk_dist_rows(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit **, uint64_t *, int32_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

static const int kTriples[5][3] = {{20, 50, 50}, {40, 60, 60}, {60, 70, 70}, {20, 40, 40}, {25, 50, 50}};   // 20/60 ties 25/75
static const uint32_t kNone = RK_MREACH_NONE;

struct Frac {   // a ratio c / u, u > 0; "none": a weight beyond every ratio
    long long c = 0, u = 1;
    bool none = false;
};
static Frac frac_of(const rk_hit &h, int metric)
{
    Frac f;
    f.c = h.common;
    f.u = metric ? std::min(h.size0, h.size1) : h.size0 + h.size1 - h.common;
    return f;
}
// a weighs less than b: the larger ratio
static bool less_weight(const Frac &a, const Frac &b)
{
    if (a.none || b.none) return !a.none && b.none;
    return a.c * b.u > b.c * a.u;
}
static Frac max_weight(const Frac &a, const Frac &b) { return less_weight(a, b) ? b : a; }
// a mark of the dist field that falls as the ratio rises, the same for equal ratios (25/75 and 20/60 are not equal as doubles)
static double mark(const rk_hit &h) { return 1.0 - std::round(4096.0 * h.common / (h.size0 + h.size1 - h.common)) / 4096.0; }

struct Out {
    std::vector<double> core_dist;
    std::vector<uint32_t> core_nb;
    std::vector<rk_hit> edges;
    explicit Out(uint32_t n) : core_dist(n, 77.0), core_nb(n, 77) {}
};
static bool same_record(const rk_hit &a, const rk_hit &b)
{
    return a.row == b.row && a.col == b.col && a.common == b.common && a.size0 == b.size0 && a.size1 == b.size1 && a.jorc == b.jorc && a.dist == b.dist;
}
static bool same(const Out &a, const Out &b, bool with_nb = true)
{
    if (a.core_dist != b.core_dist || (with_nb && a.core_nb != b.core_nb) || a.edges.size() != b.edges.size()) return false;
    for (size_t i = 0; i < a.edges.size(); i++)
        if (!same_record(a.edges[i], b.edges[i])) return false;
    return true;
}

// the rule, plainly: per genome a sorted list, then Kruskal by repeatedly taking the smallest record that joins two components
static Out plain(const std::vector<rk_hit> &hits, uint32_t n, uint32_t min_pts, int metric)
{
    Out o(n);
    const uint32_t k = min_pts - 1;
    std::vector<Frac> core(n);
    for (uint32_t v = 0; v < n; v++) {
        o.core_dist[v] = k ? INFINITY : 0.0;
        o.core_nb[v] = kNone;
        core[v].c = 1;   // k = 0: the ratio 1 / 1, the smallest weight there is
        if (!k) continue;
        std::vector<std::pair<uint32_t, size_t>> list;   // (neighbour, record)
        for (size_t e = 0; e < hits.size(); e++)
            if (hits[e].row == v || hits[e].col == v) list.push_back({hits[e].row == v ? hits[e].col : hits[e].row, e});
        std::sort(list.begin(), list.end(), [&](const std::pair<uint32_t, size_t> &a, const std::pair<uint32_t, size_t> &b) {
            const Frac fa = frac_of(hits[a.second], metric), fb = frac_of(hits[b.second], metric);
            if (fa.c * fb.u != fb.c * fa.u) return fa.c * fb.u > fb.c * fa.u;
            return a.first < b.first;
        });
        core[v].none = list.size() < k;
        if (core[v].none) continue;
        core[v] = frac_of(hits[list[k - 1].second], metric);
        o.core_dist[v] = hits[list[k - 1].second].dist;
        o.core_nb[v] = list[k - 1].first;
    }
    std::vector<uint32_t> comp(n);
    for (uint32_t v = 0; v < n; v++) comp[v] = v;
    for (;;) {
        long best = -1;
        Frac best_w;
        for (size_t e = 0; e < hits.size(); e++) {
            const rk_hit &h = hits[e];
            if (comp[h.row] == comp[h.col]) continue;
            const Frac w = max_weight(frac_of(h, metric), max_weight(core[h.row], core[h.col]));
            if (w.none) continue;
            bool better = best < 0 || less_weight(w, best_w);
            if (!better && !less_weight(best_w, w)) {
                const rk_hit &g = hits[(size_t)best];
                const uint32_t h0 = std::min(h.row, h.col), h1 = std::max(h.row, h.col), g0 = std::min(g.row, g.col), g1 = std::max(g.row, g.col);
                better = h0 != g0 ? h0 < g0 : h1 < g1;
            }
            if (better) {
                best = (long)e;
                best_w = w;
            }
        }
        if (best < 0) break;
        const uint32_t from = comp[hits[(size_t)best].row], to = comp[hits[(size_t)best].col];
        for (uint32_t v = 0; v < n; v++)
            if (comp[v] == from) comp[v] = to;
        o.edges.push_back(hits[(size_t)best]);
    }
    return o;
}

static int call(const std::vector<rk_hit> &hits, uint32_t n, uint32_t min_pts, int metric, Out *o, bool all = true)
{
    rk_hit *edges = nullptr;
    uint64_t n_edges = 0;
    const int rc = rk_mreach_hits(hits.empty() ? nullptr : hits.data(), hits.size(), n, min_pts, metric, o->core_dist.data(), all ? o->core_nb.data() : nullptr,
                                  &edges, &n_edges);
    if (rc == RK_OK) {
        o->edges.assign(edges, edges + n_edges);
        rk_free_host(edges);
    }
    return rc;
}

// the cut, plainly: labels by repeated relaxation over ALL the hits between genomes that are core at t -- the DBSCAN of the graph below t
static std::vector<uint32_t> plain_cut(const std::vector<rk_hit> &hits, const Out &o, uint32_t n, double t)
{
    std::vector<uint32_t> label(n);
    for (uint32_t v = 0; v < n; v++) label[v] = o.core_dist[v] < t ? v : RK_DBSCAN_NOISE;
    for (bool changed = true; changed;) {
        changed = false;
        for (const rk_hit &h : hits)
            if (h.dist < t && o.core_dist[h.row] < t && o.core_dist[h.col] < t && label[h.row] != label[h.col]) {
                label[h.row] = label[h.col] = std::min(label[h.row], label[h.col]);
                changed = true;
            }
    }
    return label;
}

int main()
{
    std::mt19937 rng(31);
    unsigned long n_edges_seen = 0, ties = 0, cuts = 0;
    for (int c = 0; c < 600; c++) {
        const uint32_t n = 1 + c % 24, min_pts = 1 + rng() % (n + 2);
        const int metric = c & 1;
        std::vector<rk_hit> hits;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++)
                if (rng() % (2 + c % 5) == 0) {
                    const int *t = kTriples[rng() % 5];
                    rk_hit h{i, j, t[0], t[1], t[2], 0, 0.25 + (double)hits.size(), 0.0};
                    h.dist = mark(h);   // (metric 0's ratio under both metrics: only the cut reads it, and the cut is checked under metric 0)
                    hits.push_back(h);
                }
        const Out want = plain(hits, n, min_pts, metric);
        n_edges_seen += want.edges.size();
        for (size_t i = 1; i < want.edges.size(); i++) ties += want.edges[i].dist == want.edges[i - 1].dist;
        Out got(n);
        if (call(hits, n, min_pts, metric, &got) != RK_OK || !same(got, want)) { printf("rk_mreach_hits: mismatch at case %d\n", c); return 1; }
        std::vector<rk_hit> other = hits;   // shuffled, rows and cols swapped: sizes travel with their genome
        std::shuffle(other.begin(), other.end(), rng);
        for (rk_hit &h : other) {
            std::swap(h.row, h.col);
            std::swap(h.size0, h.size1);
        }
        Out again(n);
        if (call(other, n, min_pts, metric, &again) != RK_OK) { printf("rk_mreach_hits: swapped records refused at case %d\n", c); return 1; }
        for (rk_hit &h : again.edges) {
            std::swap(h.row, h.col);
            std::swap(h.size0, h.size1);
        }
        if (!same(again, want)) { printf("rk_mreach_hits: record order matters at case %d\n", c); return 1; }
        Out two(n);   // without the optional output
        if (call(hits, n, min_pts, metric, &two, false) != RK_OK || !same(two, want, false) || two.core_nb != Out(n).core_nb) {
            printf("rk_mreach_hits: optional output at case %d\n", c);
            return 1;
        }
        // the cut at every distance that occurs, one step either side: the core labels of the graph below t
        if (metric == 0) {
            std::vector<double> ts = {0.0, 2.0};
            for (const rk_hit &h : hits) {
                ts.push_back(h.dist);
                ts.push_back(std::nextafter(h.dist, 2.0));
            }
            for (double t : ts) {
                std::vector<uint32_t> labels(n, 77);
                if (rk_mreach_cut(got.edges.empty() ? nullptr : got.edges.data(), got.edges.size(), got.core_dist.data(), n, t, labels.data()) != RK_OK ||
                    labels != plain_cut(hits, got, n, t)) {
                    printf("rk_mreach_cut: mismatch at case %d, t = %f\n", c, t);
                    return 1;
                }
                cuts++;
            }
        }
        // refusals: nothing is written
        Out r(n);
        rk_hit *edges = (rk_hit *)&r;
        uint64_t n_edges = 77;
        auto clean = [&]() { return r.core_dist == Out(n).core_dist && r.core_nb == Out(n).core_nb && edges == (rk_hit *)&r && n_edges == 77; };
        rk_hit bad[3] = {{0, n, 25, 50, 50, 0, 0, 0}, {n + 5, 0, 25, 50, 50, 0, 0, 0}, {n - 1, n - 1, 25, 50, 50, 0, 0, 0}};
        for (const rk_hit &b : bad) {
            std::vector<rk_hit> h2 = hits;
            h2.insert(h2.begin() + (long)(rng() % (h2.size() + 1)), b);
            if (rk_mreach_hits(h2.data(), h2.size(), n, min_pts, metric, r.core_dist.data(), r.core_nb.data(), &edges, &n_edges) != RK_ERR_ARG || !clean()) {
                printf("rk_mreach_hits: bad record accepted or something written at case %d\n", c);
                return 1;
            }
            std::vector<uint32_t> labels(n, 77);
            if (b.row != b.col && (rk_mreach_cut(&b, 1, want.core_dist.data(), n, 1.0, labels.data()) != RK_ERR_ARG || labels != std::vector<uint32_t>(n, 77))) {
                printf("rk_mreach_cut: bad edge accepted or something written at case %d\n", c);
                return 1;
            }
        }
        const rk_hit *hp = hits.empty() ? nullptr : hits.data();
        if (rk_mreach_hits(hp, hits.size(), n, 0, metric, r.core_dist.data(), r.core_nb.data(), &edges, &n_edges) != RK_ERR_ARG ||
            rk_mreach_hits(hp, hits.size(), n, min_pts, metric, nullptr, r.core_nb.data(), &edges, &n_edges) != RK_ERR_ARG ||
            rk_mreach_hits(hp, hits.size(), n, min_pts, metric, r.core_dist.data(), r.core_nb.data(), nullptr, &n_edges) != RK_ERR_ARG ||
            rk_mreach_hits(hp, hits.size(), n, min_pts, metric, r.core_dist.data(), r.core_nb.data(), &edges, nullptr) != RK_ERR_ARG ||
            rk_mreach_hits(nullptr, hits.size() + 1, n, min_pts, metric, r.core_dist.data(), r.core_nb.data(), &edges, &n_edges) != RK_ERR_ARG || !clean()) {
            printf("rk_mreach_hits: a refusal missed or something written at case %d\n", c);
            return 1;
        }
        std::vector<uint32_t> labels(n, 77);
        if (rk_mreach_cut(nullptr, 1, want.core_dist.data(), n, 1.0, labels.data()) != RK_ERR_ARG || rk_mreach_cut(nullptr, 0, nullptr, n, 1.0, labels.data()) != RK_ERR_ARG ||
            rk_mreach_cut(nullptr, 0, want.core_dist.data(), n, 1.0, nullptr) != RK_ERR_ARG || labels != std::vector<uint32_t>(n, 77)) {
            printf("rk_mreach_cut: a null pointer accepted or something written at case %d\n", c);
            return 1;
        }
    }
    if (n_edges_seen < 1500 || ties < 500) { printf("only %lu edges, %lu of them tied with their predecessor: the cases are too easy\n", n_edges_seen, ties); return 1; }
    rk_hit *edges = nullptr;
    uint64_t n_edges = 77;
    if (rk_mreach_hits(nullptr, 0, 0, 1, 0, nullptr, nullptr, &edges, &n_edges) != RK_OK || n_edges != 0 || !edges) return 1;   // no genome: no edge
    rk_free_host(edges);
    if (rk_mreach_cut(nullptr, 0, nullptr, 0, 1.0, nullptr) != RK_OK) return 1;
    if (rk_mreach_rows(nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr) != RK_ERR_ARG) return 1;
    printf("rk_mreach_hits, rk_mreach_cut: 600 cases clean (%lu edges, %lu tied with their predecessor, %lu cuts)\n", n_edges_seen, ties, cuts);
    return 0;
}
