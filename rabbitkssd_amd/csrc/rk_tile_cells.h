// rk_tile_cells.h -- the cells of a DIAGONAL tile of rk_tile_kernel (rk_dist_tile.inc) that can be reported: the 496 cells
// (row, col) with row < col < 32 of the 32 x 32 tile, numbered 0 .. 495 so that 512 threads evaluate them in one round.
// Plain arithmetic, shared with the host (tools/tile_cells_check.cpp, tests/test_tile_cells_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_TILE_CELLS_FN __host__ __device__ inline
#else
#define RK_TILE_CELLS_FN inline
#endif

constexpr uint32_t kTileTriCells = 496;   // 32 * 31 / 2

// Cell number `i` -> (row, col); false (row and col untouched) from 496 on.
//
// Column c holds c reportable cells (rows 0 .. c - 1), so the columns c and 32 - c together hold 32: the numbers 32 * (c - 1)
// .. 32 * (c - 1) + 31 are column c (rows ascending) followed by column 32 - c (rows ascending), c = 1 .. 15, and the last 16
// numbers are column 16.  The counts lie as cnt[col * 32 + row], a 4-byte read's bank is its row and a wave reads in two groups
// of 32 lanes (32 consecutive numbers): inside a column the rows differ, so a group's reads meet 2-way at most (the rows
// both columns hold).  No table: a shift, an add, a compare and two selects.
RK_TILE_CELLS_FN bool rk_tile_tri_cell(uint32_t i, uint32_t &row, uint32_t &col)
{
    if (i >= kTileTriCells) return false;
    const uint32_t c = (i >> 5) + 1u, j = i & 31u;   // c = 1 .. 16; at c = 16 only j < 16 passes the test above
    const bool first = j < c;
    row = first ? j : j - c;
    col = first ? c : 32u - c;
    return true;
}
