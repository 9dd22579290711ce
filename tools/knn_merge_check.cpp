// Developer check: rk_knn_hits and rk_knn_merge (host code of rk_knn.hip) against a plain sort under the host sanitizers, as a
// stand-alone program -- 400 random small graphs (n = 1 .. 24, both metrics, k = 1 .. n + 1, equal ratios from different counts):
// the lists of the whole, the fold of two parts, merge(a, a), off_out aliasing a_off, lists longer than k, and the refusals (a
// genome >= n, row == col, a record that is not incident, offsets that do not ascend, null pointers), none of which may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_knn.hip -x hip tools/knn_merge_check.cpp -o knn_merge_check && ./knn_merge_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "rk_internal.h"
// what rk_knn.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
void *rk_pinned_scratch(rk_ctx *, size_t) { return nullptr; }
uint64_t rk_host_exact_distances(rk_hit *, uint64_t, const rk_dist_opts *) { return 0; }
int rk_prim_exclusive_scan_u32(rk_ctx *, const uint32_t *, uint32_t *, uint64_t, hipStream_t) { return -1; }
extern "C" int rk_dist_rows_dev(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit *, uint64_t, uint64_t *, void *) { return -1; }
extern "C" int rk_dist_rows(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit **, uint64_t *, int32_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

static const int kTriples[5][3] = {{20, 50, 50}, {40, 60, 60}, {60, 70, 70}, {20, 40, 40}, {25, 50, 50}};   // 20/60 ties 25/75

struct Lists {
    std::vector<uint64_t> off;
    std::vector<rk_hit> rec;
};

// a before b in the list of v: integers only
static bool before(const rk_hit &a, const rk_hit &b, uint32_t v, int metric)
{
    const long long ca = a.common, cb = b.common;
    const long long ua = metric ? std::min(a.size0, a.size1) : a.size0 + a.size1 - a.common, ub = metric ? std::min(b.size0, b.size1) : b.size0 + b.size1 - b.common;
    if (ca * ub != cb * ua) return ca * ub > cb * ua;
    return (a.row == v ? a.col : a.row) < (b.row == v ? b.col : b.row);
}

static Lists plain(const std::vector<rk_hit> &hits, uint32_t n, uint32_t k, int metric)
{
    Lists l;
    l.off.push_back(0);
    for (uint32_t v = 0; v < n; v++) {
        std::vector<rk_hit> mine;
        for (const rk_hit &h : hits)
            if (h.row == v || h.col == v) mine.push_back(h);
        std::sort(mine.begin(), mine.end(), [&](const rk_hit &a, const rk_hit &b) { return before(a, b, v, metric); });
        if (mine.size() > k) mine.resize(k);
        l.rec.insert(l.rec.end(), mine.begin(), mine.end());
        l.off.push_back(l.rec.size());
    }
    return l;
}

static bool same(const rk_hit &a, const rk_hit &b)
{
    return a.row == b.row && a.col == b.col && a.common == b.common && a.size0 == b.size0 && a.size1 == b.size1 && a.jorc == b.jorc && a.dist == b.dist;
}

static bool equal(const Lists &want, const uint64_t *off, const rk_hit *rec, uint64_t n_rec)
{
    if (n_rec != want.rec.size() || (n_rec == 0) != (rec == nullptr)) return false;
    for (size_t i = 0; i < want.off.size(); i++)
        if (off[i] != want.off[i]) return false;
    for (uint64_t i = 0; i < n_rec; i++)
        if (!same(rec[i], want.rec[i])) return false;
    return true;
}

static Lists lists_of(const std::vector<rk_hit> &hits, uint32_t n, uint32_t k, int metric, bool *ok)
{
    Lists l;
    l.off.assign((size_t)n + 1, 99);
    rk_hit *out = nullptr;
    uint64_t n_out = 0;
    *ok = rk_knn_hits(hits.empty() ? nullptr : hits.data(), hits.size(), n, k, metric, l.off.data(), &out, &n_out) == RK_OK;
    if (*ok) *ok = equal(plain(hits, n, k, metric), l.off.data(), out, n_out);
    if (out) l.rec.assign(out, out + n_out);
    rk_free_host(out);
    return l;
}

int main()
{
    std::mt19937 rng(28);
    for (int c = 0; c < 400; c++) {
        const uint32_t n = 1 + c % 24, k = 1 + rng() % (n + 1);
        const int metric = c & 1;
        std::vector<rk_hit> hits, part[2];
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++)
                if (rng() % 3 == 0) {
                    const int *t = kTriples[rng() % 5];
                    hits.push_back(rk_hit{i, j, t[0], t[1], t[2], 0, 0.25 + (double)hits.size(), 0.5 + (double)hits.size()});
                    part[rng() % 2].push_back(hits.back());
                    if (rng() % 8 == 0) part[rng() % 2].push_back(hits.back());   // (possibly in both parts)
                }
        std::shuffle(hits.begin(), hits.end(), rng);
        bool ok = true;
        const Lists whole = lists_of(hits, n, k, metric, &ok);
        if (!ok) { printf("rk_knn_hits: mismatch at case %d\n", c); return 1; }
        Lists p[2];
        for (int s = 0; s < 2; s++) {   // (one record per pair inside a part)
            std::sort(part[s].begin(), part[s].end(), [](const rk_hit &a, const rk_hit &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
            part[s].erase(std::unique(part[s].begin(), part[s].end(), [](const rk_hit &a, const rk_hit &b) { return a.row == b.row && a.col == b.col; }), part[s].end());
            p[s] = lists_of(part[s], n, s ? k : n, metric, &ok);   // part 0 with lists longer than k
            if (!ok) { printf("rk_knn_hits: mismatch at part %d of case %d\n", s, c); return 1; }
        }
        const Lists want = plain(hits, n, k, metric);
        std::vector<uint64_t> off((size_t)n + 1, 99);
        rk_hit *out = nullptr;
        uint64_t n_out = 0;
        if (rk_knn_merge(p[0].off.data(), p[0].rec.data(), p[1].off.data(), p[1].rec.data(), n, k, metric, off.data(), &out, &n_out) != RK_OK || !equal(want, off.data(), out, n_out)) {
            printf("rk_knn_merge: mismatch at case %d\n", c);
            return 1;
        }
        rk_free_host(out);
        if (rk_knn_merge(whole.off.data(), whole.rec.data(), whole.off.data(), whole.rec.data(), n, k, metric, off.data(), &out, &n_out) != RK_OK || !equal(want, off.data(), out, n_out)) {
            printf("rk_knn_merge(a, a): mismatch at case %d\n", c);
            return 1;
        }
        rk_free_host(out);
        std::vector<uint64_t> alias = p[0].off;   // off_out aliasing a_off
        if (rk_knn_merge(alias.data(), p[0].rec.data(), p[1].off.data(), p[1].rec.data(), n, k, metric, alias.data(), &out, &n_out) != RK_OK || !equal(want, alias.data(), out, n_out)) {
            printf("rk_knn_merge: alias mismatch at case %d\n", c);
            return 1;
        }
        rk_free_host(out);
        // refusals: nothing is written
        if (!whole.rec.empty()) {
            const rk_hit good = whole.rec[0];
            const uint32_t v = (uint32_t)(std::upper_bound(whole.off.begin(), whole.off.end(), (uint64_t)0) - whole.off.begin() - 1);   // the genome that owns record 0
            rk_hit bad[4] = {good, good, good, good};
            bad[0].col = n;
            bad[1].row = bad[1].col;
            bad[2].row = bad[2].col = v;
            bad[3].row = std::min((v + 1) % n, (v + 2) % n);   // two genomes other than v: not incident to it (n >= 3)
            bad[3].col = std::max((v + 1) % n, (v + 2) % n);
            for (int b = 0; b < (n >= 3 ? 4 : 3); b++) {
                Lists broken = whole;
                broken.rec[0] = bad[b];
                std::fill(off.begin(), off.end(), 99);
                out = (rk_hit *)&off;
                n_out = 99;
                if (rk_knn_merge(broken.off.data(), broken.rec.data(), whole.off.data(), whole.rec.data(), n, k, metric, off.data(), &out, &n_out) != RK_ERR_ARG ||
                    rk_knn_merge(whole.off.data(), whole.rec.data(), broken.off.data(), broken.rec.data(), n, k, metric, off.data(), &out, &n_out) != RK_ERR_ARG ||
                    out != (rk_hit *)&off || n_out != 99 || std::count(off.begin(), off.end(), 99) != (long)off.size()) {
                    printf("rk_knn_merge: bad record %d accepted or something written at case %d\n", b, c);
                    return 1;
                }
                std::vector<rk_hit> h2 = hits;
                h2.push_back(bad[b]);
                if (b < 3 && rk_knn_hits(h2.data(), h2.size(), n, k, metric, off.data(), &out, &n_out) != RK_ERR_ARG) { printf("rk_knn_hits: bad record accepted\n"); return 1; }
            }
            Lists broken = whole;
            broken.off[v] = broken.off[v + 1] + 1;   // the offsets step down behind v
            if (rk_knn_merge(broken.off.data(), broken.rec.data(), whole.off.data(), whole.rec.data(), n, k, metric, off.data(), &out, &n_out) != RK_ERR_ARG) {
                printf("rk_knn_merge: descending offsets accepted at case %d\n", c);
                return 1;
            }
        }
    }
    uint64_t zero[4] = {0, 0, 0, 0}, off[4], n_out = 0;
    rk_hit *out = nullptr;
    if (rk_knn_merge(nullptr, nullptr, zero, nullptr, 3, 2, 0, off, &out, &n_out) != RK_ERR_ARG) return 1;
    if (rk_knn_merge(zero, nullptr, nullptr, nullptr, 3, 2, 0, off, &out, &n_out) != RK_ERR_ARG) return 1;
    if (rk_knn_merge(zero, nullptr, zero, nullptr, 3, 2, 0, nullptr, &out, &n_out) != RK_ERR_ARG) return 1;
    if (rk_knn_merge(zero, nullptr, zero, nullptr, 3, 2, 0, off, nullptr, &n_out) != RK_ERR_ARG) return 1;
    if (rk_knn_merge(zero, nullptr, zero, nullptr, 3, 2, 0, off, &out, nullptr) != RK_ERR_ARG) return 1;
    if (rk_knn_merge(zero, nullptr, zero, nullptr, 3, 2, 0, off, &out, &n_out) != RK_OK || out || n_out) return 1;
    if (rk_knn_hits(nullptr, 1, 3, 2, 0, off, &out, &n_out) != RK_ERR_ARG || rk_knn_hits(nullptr, 0, 3, 2, 0, nullptr, &out, &n_out) != RK_ERR_ARG) return 1;
    if (rk_knn_hits(nullptr, 0, 3, 2, 0, off, nullptr, &n_out) != RK_ERR_ARG || rk_knn_hits(nullptr, 0, 3, 2, 0, off, &out, nullptr) != RK_ERR_ARG) return 1;
    if (rk_knn_rows(nullptr, nullptr, nullptr, 3, off, &out, &n_out, nullptr) != RK_ERR_ARG) return 1;
    printf("rk_knn_hits, rk_knn_merge: 400 cases clean\n");
    return 0;
}
