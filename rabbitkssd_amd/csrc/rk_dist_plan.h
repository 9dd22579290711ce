// rk_dist_plan.h -- host arithmetic the distance joins share (rk_dist.hip, rk_distq.hip, and rk_edge_stage.h for rk_cluster.hip,
// rk_forest.hip and rk_greedy.hip): the prefilter threshold, the rows of a row shard, the first capacity of a hit buffer, the
// widening of the device's threshold.  Nothing here launches or allocates, and everything compiles without HIP (tools/dist_plan_check.cpp, tests/test_dist_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "rabbitkssd.h"

// The device reports with a threshold wider by this much, relative (~64 ulps: orders beyond the 2 ulps between the device's log and
// the C library's), and the host decides exactly: rk_dist_rows every record, rk_edge_stage.h those within it of the threshold.
constexpr double kBorderRel = 0x1p-46;

// distance < D  <=>  jaccard > t/(2-t), t = exp(-k D)   (containment: c > t); 1e-6 relative slack
// keeps the reject conservative, the exact formula still decides.  (Callers disable it -- 0.0 -- in dense mode and for D <= 0.)
inline double rk_min_jorc(const rk_dist_opts *o)
{
    const double t = exp(-(double)o->kmer_size * o->max_dist);
    return ((o->metric != 0) ? t : t / (2.0 - t)) * (1.0 - 1e-6);
}

// Row distribution: blocks of row_block consecutive rows dealt round-robin to row_step shards; this shard owns blocks row_first,
// row_first + row_step, ...  all_rows_block: what row_block becomes when the shard is all rows (every block is this shard's,
// so the caller may pick the size that suits it); 0: no override.
struct RowShard {
    uint32_t row_first = 0, row_step = 1, row_block = 1;
    uint64_t n = 0;   // rows dealt out
    RowShard() = default;
    RowShard(const rk_dist_opts *o, uint64_t n_rows, uint32_t all_rows_block)
        : row_first(o->row_first), row_step(o->row_step ? o->row_step : 1), row_block(o->row_block > 0 ? (uint32_t)o->row_block : 1), n(n_rows)
    {
        if (all_rows_block && row_step == 1 && row_first == 0) row_block = all_rows_block;
    }
    uint64_t n_blocks() const { return (n + row_block - 1) / row_block; }
    uint64_t my_blocks() const { return row_first < n_blocks() ? (n_blocks() - row_first + row_step - 1) / row_step : 0; }
    // rows of this shard: whole blocks, but for the last block of all when it is this shard's
    uint64_t n_rows() const
    {
        const uint64_t nb = n_blocks(), mine = my_blocks();
        return mine * row_block - (mine && (nb - 1 - row_first) % row_step == 0 ? nb * row_block - n : 0);
    }
};

// first capacity of a sparse join's hit buffer (an overflow is answered by a second join with the exact count)
inline uint64_t rk_hit_capacity(uint64_t n_rows) { return std::max<uint64_t>(1 << 16, n_rows * 64); }
