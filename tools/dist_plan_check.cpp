// Developer check: the host arithmetic of rk_dist_plan.h as a stand-alone program (plain C++, no HIP, no GPU) -- prints RowShard's
// counts and rk_min_jorc over a grid of cases; tests/test_dist_plan_cpu.py compares them with the loops and the expression they replaced.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -Iinclude -Irabbitkssd_amd/csrc tools/dist_plan_check.cpp -o dist_plan_check && ./dist_plan_check
#include <cstdio>
#include "rk_dist_plan.h"
int main()
{
    const uint64_t ns[] = {0, 1, 15, 16, 17, 1000};
    const uint32_t steps[] = {0, 1, 2, 3, 8};
    const int32_t blocks[] = {0, 1, 2, 16};
    for (uint64_t n : ns)
        for (uint32_t step : steps)
            for (uint32_t first : {0u, 1u, step - 1, step})
                for (int32_t block : blocks)
                    for (uint32_t all_rows : {0u, 16u, (uint32_t)n}) {   // no override, the kernels', the capacity rules'
                        if (first == 0xFFFFFFFFu) continue;   // (row_step 0: no row_step - 1)
                        rk_dist_opts o = {};
                        o.row_first = first;
                        o.row_step = step;
                        o.row_block = block;
                        const RowShard s(&o, n, all_rows);
                        printf("rows %llu %u %u %d %u : %llu %llu %llu\n", (unsigned long long)n, step, first, block, all_rows,
                               (unsigned long long)s.n_rows(), (unsigned long long)s.my_blocks(), (unsigned long long)rk_hit_capacity(s.n_rows()));
                    }
    for (int k : {10, 21})
        for (double D : {0.05, 0.3, 1.0})
            for (int metric : {0, 1}) {
                rk_dist_opts o = {};
                o.kmer_size = k;
                o.max_dist = D;
                o.metric = metric;
                printf("jorc %d %a %d : %a\n", k, D, metric, rk_min_jorc(&o));
            }
    return 0;
}
