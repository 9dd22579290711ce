// rk_query_host.h -- the host side that the consumers of query sketches share around their rules (rk_lca.hip, rk_screen.hip,
// rk_gather.hip; not part of the public ABI).  The device side is rk_query_dev.h.  Nothing here launches or allocates on the device,
// and everything compiles without HIP.  DESIGN.md 4.19.
//
//   rows      RowSel: the rows of a row shard, listed;
//   lists     prepare_lists: exported posting lists as the host rules take them;
//   result    RowsResult: off[Q + 1], a few per-row arrays and the records of a call, wherever they lie -- in a host result, in the
//             one block that comes home from the device (from_block), or nowhere (nothing ran); hand_out gives them to the caller.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rabbitkssd.h"

namespace {

// The selected rows of Q, ascending: blocks of row_block consecutive rows dealt round-robin to row_step shards, this shard owns blocks
// row_first, row_first + row_step, ... (a step or a block of 0 counts as 1) -- as rk_distq_kernel deals its row slots (RowShard)
struct RowSel {
    std::vector<uint32_t> rows;
    RowSel(uint32_t row_first, uint32_t row_step, uint32_t row_block, uint32_t Q)
    {
        const uint64_t rb = row_block ? row_block : 1, rs = row_step ? row_step : 1;
        for (uint64_t blk = row_first; blk * rb < Q; blk += rs)
            for (uint64_t r = blk * rb; r < std::min<uint64_t>(Q, (blk + 1) * rb); r++) rows.push_back((uint32_t)r);
    }
};

// lists as exported: their offsets, and a sorted copy without repeats where a list does not ascend strictly.  RK_ERR_ARG for a posting >= n_ref.
inline int prepare_lists(const uint32_t *postings, const uint32_t *counts, uint64_t n_lists, uint32_t n_ref, std::vector<uint64_t> *pos,
                         std::vector<uint32_t> *fixed, const uint32_t **post)
{
    pos->assign((size_t)n_lists + 1, 0);
    bool ascending = true;
    for (uint64_t u = 0; u < n_lists; u++) (*pos)[u + 1] = (*pos)[u] + counts[u];
    for (uint64_t u = 0; u < n_lists; u++)
        for (uint64_t i = (*pos)[u]; i < (*pos)[u + 1]; i++) {
            if (postings[i] >= n_ref) return RK_ERR_ARG;
            if (i > (*pos)[u] && postings[i - 1] >= postings[i]) ascending = false;
        }
    *post = postings;
    if (ascending) return RK_OK;
    std::vector<uint64_t> npos((size_t)n_lists + 1, 0);
    fixed->clear();
    std::vector<uint32_t> list;
    for (uint64_t u = 0; u < n_lists; u++) {
        list.assign(postings + (*pos)[u], postings + (*pos)[u + 1]);
        std::sort(list.begin(), list.end());
        list.erase(std::unique(list.begin(), list.end()), list.end());
        fixed->insert(fixed->end(), list.begin(), list.end());
        npos[u + 1] = fixed->size();
    }
    pos->swap(npos);
    *post = fixed->data();
    return RK_OK;
}

// What a call over Q rows found, as a view: off[Q + 1], N arrays of Q entries each (an unselected row's entry is never read) and the
// records.  off == null: nothing ran, every row is empty.
template <class Rec, int N> struct RowsResult {
    const uint64_t *off = nullptr;
    const uint32_t *per_row[N] = {};
    const Rec *recs = nullptr;
    uint64_t n_recs = 0;

    // the block of a device leg: off u64[Q + 1] | N arrays u32[Q] (+ 4 bytes when N Q is odd) | the records
    static size_t head_bytes(uint32_t Q) { return ((size_t)Q + 1) * 8 + (((size_t)Q * 4 * N + 7) & ~(size_t)7); }
    static RowsResult from_block(const unsigned char *b, uint32_t Q, uint64_t n_recs)
    {
        RowsResult r;
        r.off = (const uint64_t *)b;
        for (int k = 0; k < N; k++) r.per_row[k] = (const uint32_t *)(b + ((size_t)Q + 1) * 8) + (size_t)k * Q;
        r.recs = (const Rec *)(b + head_bytes(Q));
        r.n_recs = n_recs;
        return r;
    }
};

// the outputs of an entry point: the offsets, the per-row arrays at the selected rows (the others stay the caller's) and the records
// in memory of their own (rk_free_host; null without one).  RK_ERR_NOMEM leaves everything untouched.
template <class Rec, int N>
int hand_out(const RowsResult<Rec, N> &r, const RowSel &sel, uint32_t Q, uint64_t *off_out, Rec **recs_out, uint64_t *n_recs, uint32_t *const (&per_row_out)[N])
{
    Rec *p = nullptr;
    if (r.n_recs) {
        p = (Rec *)malloc(r.n_recs * sizeof(Rec));
        if (!p) return RK_ERR_NOMEM;
        memcpy(p, r.recs, r.n_recs * sizeof(Rec));
    }
    if (r.off) memcpy(off_out, r.off, ((size_t)Q + 1) * 8);
    else memset(off_out, 0, ((size_t)Q + 1) * 8);
    for (const uint32_t q : sel.rows)
        for (int k = 0; k < N; k++) per_row_out[k][q] = r.off ? r.per_row[k][q] : 0u;
    *recs_out = p;
    *n_recs = r.n_recs;
    return RK_OK;
}

}  // namespace
