// Developer check: rk_medoid_hits, rk_medoid_merge and rk_medoid_pick (host code of rk_medoid.hip) against a plain restatement of the
// rule under the host sanitizers, as a stand-alone program -- 600 random small graphs (n = 1 .. 24, both metrics, labels below n that need
// not be members, unlabelled genomes, equal ratios from different counts), each also in shuffled record order with rows and cols
// swapped, without the record arrays, split in three and folded again (out aliasing a), and the refusals (a genome >= n, row == col, a
// label that names nothing, a record outside 0 < common <= u, null pointers, an entry that is not a pair of its genome), none of which
// may write.
// No GPU call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_medoid.hip -x hip tools/medoid_hits_check.cpp -o medoid_hits_check && ./medoid_hits_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "rk_internal.h"
// what rk_medoid.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
void *rk_pinned_scratch(rk_ctx *, size_t) { return nullptr; }
uint64_t rk_host_exact_distances(rk_hit *, uint64_t, const rk_dist_opts *) { return 0; }
extern "C" int rk_dist_rows_dev(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit *, uint64_t, uint64_t *, void *) { return -1; }
extern "C" int rk_dist_rows(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit **, uint64_t *, int32_t *) { return -1; }
extern "C" void rk_free_host(void *p) { free(p); }

static const int kTriples[5][3] = {{20, 50, 50}, {40, 60, 60}, {60, 70, 70}, {20, 40, 40}, {25, 50, 50}};   // 20/60 ties 25/75
static const uint32_t kNone = RK_MEDOID_NONE;
static const rk_hit kMark = {77, 77, 77, 77, 77, 77, 7.0, 7.0};

static bool same_hit(const rk_hit &a, const rk_hit &b) { return memcmp(&a, &b, sizeof a) == 0; }

struct Out {
    std::vector<uint32_t> in_deg, out_deg;
    std::vector<uint64_t> central;
    std::vector<rk_hit> far_in, near_out;
    explicit Out(uint32_t n) : in_deg(n, 77), out_deg(n, 77), central(n, 77), far_in(n, kMark), near_out(n, kMark) {}
    rk_medoid_genomes g(bool records = true)
    {
        return rk_medoid_genomes{in_deg.data(), out_deg.data(), central.data(), records ? far_in.data() : nullptr, records ? near_out.data() : nullptr};
    }
    bool sums_equal(const Out &o) const { return in_deg == o.in_deg && out_deg == o.out_deg && central == o.central; }
    bool operator==(const Out &o) const
    {
        return sums_equal(o) && std::equal(far_in.begin(), far_in.end(), o.far_in.begin(), same_hit) && std::equal(near_out.begin(), near_out.end(), o.near_out.begin(), same_hit);
    }
};

static long long u_of(const rk_hit &h, int metric) { return metric ? std::min(h.size0, h.size1) : (long long)h.size0 + h.size1 - h.common; }
// the sign of ratio(a) - ratio(b): integers only
static int cross(const rk_hit &a, const rk_hit &b, int metric)
{
    const long long l = a.common * u_of(b, metric), r = b.common * u_of(a, metric);
    return l < r ? -1 : l > r ? 1 : 0;
}
static uint32_t nb(const rk_hit &h, uint32_t v) { return h.row == v ? h.col : h.row; }

// the rule, plainly: per genome a walk over every record
static Out plain(const std::vector<rk_hit> &hits, uint32_t n, const std::vector<uint32_t> &label, int metric)
{
    Out o(n);
    for (uint32_t v = 0; v < n; v++) {
        o.in_deg[v] = o.out_deg[v] = 0;
        o.central[v] = 0;
        o.far_in[v] = o.near_out[v] = rk_hit{kNone, kNone, 0, 0, 0, 0, 0.0, 0.0};
        for (const rk_hit &h : hits) {
            if (h.row != v && h.col != v) continue;
            const bool inside = label[h.row] == label[h.col] && label[h.row] != kNone;
            if (inside) {
                o.in_deg[v]++;
                o.central[v] += (uint64_t)(((unsigned __int128)h.common << 32) / (unsigned __int128)u_of(h, metric));
                const rk_hit &best = o.far_in[v];
                const int c = best.row == kNone ? -1 : cross(h, best, metric);
                if (c < 0 || (!c && nb(h, v) < nb(best, v))) o.far_in[v] = h;
            } else {
                o.out_deg[v]++;
                const rk_hit &best = o.near_out[v];
                const int c = best.row == kNone ? 1 : cross(h, best, metric);
                if (c > 0 || (!c && nb(h, v) < nb(best, v))) o.near_out[v] = h;
            }
        }
    }
    return o;
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int check_pick(const std::vector<rk_hit> &hits, uint32_t n, const std::vector<uint32_t> &label, int metric, Out &got, int c)
{
    rk_medoid_cluster *cl = nullptr;
    uint32_t n_cl = 0;
    const rk_medoid_genomes g = got.g();
    if (rk_medoid_pick(label.data(), &g, n, metric, &cl, &n_cl) != RK_OK) FAIL("rk_medoid_pick failed at case %d", c);
    uint32_t k = 0;
    for (uint32_t l = 0; l < n; l++) {
        uint32_t size = 0, medoid = kNone;
        uint64_t in_edges = 0;
        for (uint32_t v = 0; v < n; v++)
            if (label[v] == l) {
                size++;
                if (medoid == kNone || got.central[v] > got.central[medoid]) medoid = v;
            }
        if (!size) continue;
        const rk_hit *weak = nullptr, *near = nullptr;   // over EVERY record of the cluster
        for (const rk_hit &h : hits) {
            const bool ra = label[h.row] == l, rb = label[h.col] == l;
            if (ra && rb) {
                in_edges++;
                const int s = weak ? cross(h, *weak, metric) : -1;
                if (s < 0 || (!s && (h.row != weak->row ? h.row < weak->row : h.col < weak->col))) weak = &h;
            } else if (ra != rb) {
                const int s = near ? cross(h, *near, metric) : 1;
                if (s > 0 || (!s && (h.row != near->row ? h.row < near->row : h.col < near->col))) near = &h;
            }
        }
        if (k >= n_cl) FAIL("rk_medoid_pick: too few clusters at case %d", c);
        const rk_medoid_cluster &x = cl[k++];
        if (x.label != l || x.size != size || x.medoid != medoid || x.pad_ != 0 || x.in_edges != in_edges || x.central != got.central[medoid] ||
            (weak ? !same_hit(x.weakest_in, *weak) : x.weakest_in.row != kNone) || (near ? !same_hit(x.nearest_out, *near) : x.nearest_out.row != kNone))
            FAIL("rk_medoid_pick: cluster %u at case %d", l, c);
    }
    if (k != n_cl) FAIL("rk_medoid_pick: too many clusters at case %d", c);
    rk_free_host(cl);
    return 0;
}

int main()
{
    std::mt19937 rng(31);
    unsigned long ties = 0, moved = 0;
    for (int c = 0; c < 600; c++) {
        const uint32_t n = 1 + c % 24;
        const int metric = c & 1;
        std::vector<rk_hit> hits;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++)
                if (rng() % (2 + c % 5) == 0) {
                    const int *t = kTriples[rng() % 5];
                    hits.push_back(rk_hit{i, j, t[0], t[1], t[2], 0, 0.25 + (double)hits.size(), 0.5 + (double)hits.size()});
                }
        std::vector<uint32_t> label(n);
        const uint32_t kinds = 1 + rng() % n;
        for (uint32_t v = 0; v < n; v++) label[v] = rng() % 5 == 0 ? kNone : (uint32_t)((rng() % kinds) * 7 % n);   // (not members, as a rule)
        const Out want = plain(hits, n, label, metric);
        for (uint32_t v = 0; v < n; v++) {
            unsigned at_far = 0;
            for (const rk_hit &h : hits)
                at_far += (h.row == v || h.col == v) && want.far_in[v].row != kNone && label[h.row] == label[h.col] && label[h.row] != kNone && !cross(h, want.far_in[v], metric);
            ties += at_far > 1;
        }
        Out got(n);
        rk_medoid_genomes g = got.g();
        if (rk_medoid_hits(hits.empty() ? nullptr : hits.data(), hits.size(), n, label.data(), metric, &g) != RK_OK || !(got == want)) FAIL("rk_medoid_hits: mismatch at case %d", c);
        if (check_pick(hits, n, label, metric, got, c)) return 1;
        for (uint32_t v = 0; v < n; v++) moved += label[v] != kNone && got.central[v] > 0;
        std::vector<rk_hit> other = hits;   // shuffled, rows and cols swapped: sizes travel with their genome, the records come back row first
        std::shuffle(other.begin(), other.end(), rng);
        for (rk_hit &h : other) {
            std::swap(h.row, h.col);
            std::swap(h.size0, h.size1);
        }
        Out again(n);
        g = again.g();
        if (rk_medoid_hits(other.data(), other.size(), n, label.data(), metric, &g) != RK_OK || !(again == want)) FAIL("rk_medoid_hits: record order matters at case %d", c);
        Out bare(n);   // without the record arrays
        g = bare.g(false);
        if (rk_medoid_hits(hits.data(), hits.size(), n, label.data(), metric, &g) != RK_OK || !bare.sums_equal(want) || !(Out(n).far_in.size() == n) ||
            !std::equal(bare.far_in.begin(), bare.far_in.end(), Out(n).far_in.begin(), same_hit) || !std::equal(bare.near_out.begin(), bare.near_out.end(), Out(n).near_out.begin(), same_hit))
            FAIL("rk_medoid_hits: optional outputs at case %d", c);
        // three disjoint parts, folded: (a + b) + c into a itself
        std::vector<rk_hit> part[3];
        for (const rk_hit &h : hits) part[rng() % 3].push_back(h);
        Out p0(n), p1(n), p2(n);
        Out *ps[3] = {&p0, &p1, &p2};
        for (int k = 0; k < 3; k++) {
            g = ps[k]->g();
            if (rk_medoid_hits(part[k].data(), part[k].size(), n, label.data(), metric, &g) != RK_OK) FAIL("rk_medoid_hits: a part at case %d", c);
        }
        rk_medoid_genomes ga = p0.g(), gb = p1.g(), gc = p2.g();
        if (rk_medoid_merge(&ga, &gb, n, metric, &ga) != RK_OK || rk_medoid_merge(&ga, &gc, n, metric, &ga) != RK_OK || !(p0 == want)) FAIL("rk_medoid_merge: the fold differs at case %d", c);
        // refusals: nothing is written
        const Out clean(n);
        Out r(n);
        g = r.g();
        rk_hit bad[5] = {{0, n, 25, 50, 50, 0, 0, 0}, {n + 5, 0, 25, 50, 50, 0, 0, 0}, {n - 1, n - 1, 25, 50, 50, 0, 0, 0}, {0, n > 1 ? 1u : 0u, 0, 50, 50, 0, 0, 0},
                         {0, n > 1 ? 1u : 0u, 60, 50, 50, 0, 0, 0}};
        for (int k = 0; k < 5; k++) {
            if (k >= 3 && n < 2) continue;
            std::vector<rk_hit> h2 = hits;
            h2.insert(h2.begin() + (long)(rng() % (h2.size() + 1)), bad[k]);
            if (rk_medoid_hits(h2.data(), h2.size(), n, label.data(), metric, &g) != (k < 3 ? RK_ERR_ARG : RK_ERR_UNSUPPORTED) || !(r == clean))
                FAIL("rk_medoid_hits: bad record %d accepted or something written at case %d", k, c);
        }
        std::vector<uint32_t> wrong = label;
        wrong[rng() % n] = n + rng() % 3;
        rk_medoid_cluster *cl = nullptr;
        uint32_t n_cl = 77;
        if (rk_medoid_hits(hits.data(), hits.size(), n, wrong.data(), metric, &g) != RK_ERR_ARG || rk_medoid_pick(wrong.data(), &g, n, metric, &cl, &n_cl) != RK_ERR_ARG || cl ||
            n_cl != 77 || !(r == clean))
            FAIL("a label beyond n accepted or something written at case %d", c);
        rk_medoid_genomes lone = r.g();
        lone.central = nullptr;
        if (rk_medoid_hits(hits.data(), hits.size(), n, label.data(), metric, &lone) != RK_ERR_ARG || rk_medoid_hits(hits.data(), hits.size(), n, nullptr, metric, &g) != RK_ERR_ARG ||
            rk_medoid_hits(nullptr, hits.size() + 1, n, label.data(), metric, &g) != RK_ERR_ARG || rk_medoid_hits(hits.data(), hits.size(), n, label.data(), metric, nullptr) != RK_ERR_ARG ||
            rk_medoid_merge(&ga, &lone, n, metric, &g) != RK_ERR_ARG || rk_medoid_merge(nullptr, &ga, n, metric, &g) != RK_ERR_ARG || !(r == clean))
            FAIL("a null pointer accepted or something written at case %d", c);
        Out spoiled = want;   // an entry that is not a pair of its genome
        spoiled.near_out[0] = rk_hit{n, n + 1, 25, 50, 50, 0, 0, 0};
        rk_medoid_genomes gs = spoiled.g();
        if (rk_medoid_merge(&gs, &gb, n, metric, &g) != RK_ERR_ARG || rk_medoid_merge(&gb, &gs, n, metric, &g) != RK_ERR_ARG || !(r == clean))
            FAIL("rk_medoid_merge: a foreign record accepted or something written at case %d", c);
    }
    if (ties < 300 || moved < 1000) FAIL("only %lu ties and %lu central genomes: the cases are too easy", ties, moved);
    rk_medoid_genomes none{};
    rk_medoid_cluster *cl = nullptr;
    uint32_t n_cl = 0;
    if (rk_medoid_hits(nullptr, 0, 0, nullptr, 0, &none) != RK_OK || rk_medoid_merge(&none, &none, 0, 0, &none) != RK_OK || rk_medoid_pick(nullptr, &none, 0, 0, &cl, &n_cl) != RK_OK || cl)
        FAIL("no genome: something but RK_OK");
    if (rk_medoid_rows(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != RK_ERR_ARG) return 1;
    printf("rk_medoid_hits, rk_medoid_merge, rk_medoid_pick: 600 cases clean (%lu extremes decided by a tie)\n", ties);
    return 0;
}
