// Developer check: rk_cluster_merge (host code of rk_cluster.hip) against a plain union-find under the host sanitizers, as a
// stand-alone program -- 200 random pairs of partitions, n = 1 .. 500, out aliasing a, an entry >= n, null pointers.  No GPU
// call is made: a CPU check, not for a GPU machine.  The rest of the library is stubbed below.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Irabbitkssd_amd/csrc \
//         rabbitkssd_amd/csrc/rk_cluster.hip -x hip tools/cluster_merge_check.cpp -o cluster_merge_check && ./cluster_merge_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include <algorithm>
#include <numeric>
#include "rk_internal.h"
// what rk_cluster.hip references from the rest of the library (never reached here)
int rk_fail(rk_ctx *, int code, const char *, ...) { return code; }
void *rk_pool_alloc(rk_ctx *, size_t) { return nullptr; }
void rk_pool_free(rk_ctx *, void *) {}
void *rk_pinned_scratch(rk_ctx *, size_t) { return nullptr; }
uint64_t rk_host_exact_distances(rk_hit *, uint64_t, const rk_dist_opts *) { return 0; }
extern "C" int rk_index_order(const rk_index *, uint32_t *) { return -1; }
extern "C" int rk_dist_rows_dev(rk_ctx *, const rk_index *, const rk_sketches *, const rk_dist_opts *, rk_hit *, uint64_t, uint64_t *, void *) { return -1; }
static uint32_t root(std::vector<uint32_t> &p, uint32_t x) { while (p[x] != x) x = p[x] = p[p[x]]; return x; }
static std::vector<uint32_t> canon(std::vector<std::pair<uint32_t, uint32_t>> e, uint32_t n) {
    std::vector<uint32_t> p(n); std::iota(p.begin(), p.end(), 0u);
    for (auto &x : e) { uint32_t a = root(p, x.first), b = root(p, x.second); if (a != b) p[std::max(a, b)] = std::min(a, b); }
    for (uint32_t i = 0; i < n; i++) p[i] = root(p, i);
    return p;
}
int main() {
    std::mt19937 rng(20);
    for (int c = 0; c < 200; c++) {
        uint32_t n = 1 + c * 499 / 199;
        auto part = [&]() { std::vector<std::pair<uint32_t, uint32_t>> e(rng() % (2 * n)); for (auto &x : e) x = {rng() % n, rng() % n}; return canon(e, n); };
        std::vector<uint32_t> a = part(), b = part(), out(n);
        std::vector<std::pair<uint32_t, uint32_t>> e;
        for (uint32_t i = 0; i < n; i++) { e.push_back({i, a[i]}); e.push_back({i, b[i]}); }
        auto want = canon(e, n);
        if (rk_cluster_merge(a.data(), b.data(), n, out.data()) != 0 || out != want) { printf("mismatch at case %d\n", c); return 1; }
        if (rk_cluster_merge(a.data(), b.data(), n, a.data()) != 0 || a != want) { printf("alias mismatch at case %d\n", c); return 1; }
        b[n - 1] = n;
        if (rk_cluster_merge(a.data(), b.data(), n, out.data()) != RK_ERR_ARG) { printf("entry >= n accepted\n"); return 1; }
    }
    if (rk_cluster_merge(nullptr, nullptr, 3, nullptr) != RK_ERR_ARG) return 1;
    printf("rk_cluster_merge: 200 cases clean\n");
    return 0;
}
