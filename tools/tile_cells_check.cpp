// Developer check: rk_tile_cells.h (the numbering of a diagonal tile's reportable cells in rk_tile_kernel) as a stand-alone
// program (plain C++, no HIP, no GPU).  It checks the map itself -- a bijection from 0 .. 495 onto {row < col < 32}, 496 .. 1023
// rejected with row and col untouched, the rounds of 256 / 512 / 1,024 threads cover every cell exactly once, a group of 32
// lanes reads no bank (= row) of cnt[col * 32 + row] more than twice -- and prints every number's answer, which
// tests/test_tile_cells_cpu.py checks again on its own.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -Irabbitkssd_amd/csrc tools/tile_cells_check.cpp -o tile_cells_check && ./tile_cells_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rk_tile_cells.h"

static void fail(const char *what, uint32_t i)
{
    fprintf(stderr, "tile_cells_check: %s at %u\n", what, i);
    exit(1);
}

int main()
{
    constexpr uint32_t kUntouched = 0xDEADu;
    // ---- the map: every number's answer, a bijection below 496, nothing from 496 on
    std::vector<int> seen(32 * 32, 0);
    for (uint32_t i = 0; i < 1024; i++) {
        uint32_t row = kUntouched, col = kUntouched;
        const bool ok = rk_tile_tri_cell(i, row, col);
        printf("cell %u %d %u %u\n", i, ok ? 1 : 0, row, col);
        if (ok != (i < kTileTriCells)) fail("accepted / rejected on the wrong side of 496", i);
        if (!ok) {
            if (row != kUntouched || col != kUntouched) fail("a rejected number wrote row or col", i);
            continue;
        }
        if (!(row < col && col < 32)) fail("not a cell above the diagonal", i);
        if (seen[col * 32 + row]++) fail("a cell twice", i);
    }
    uint32_t n_seen = 0;
    for (uint32_t col = 0; col < 32; col++)
        for (uint32_t row = 0; row < 32; row++) {
            if (seen[col * 32 + row] != (row < col ? 1 : 0)) fail("a cell of the wrong side, or a missing one", col * 32 + row);
            n_seen += (uint32_t)seen[col * 32 + row];
        }
    if (n_seen != kTileTriCells) fail("cells", n_seen);
    // ---- the rounds of the kernel's evaluation loop: thread t of round r holds number r * threads + t
    for (uint32_t threads : {256u, 512u, 1024u}) {
        const uint32_t rounds = (kTileTriCells + threads - 1) / threads;
        if (rounds != (threads == 256 ? 2u : 1u)) fail("rounds", threads);
        std::vector<int> hit(32 * 32, 0);
        uint32_t n_hit = 0;
        for (uint32_t r = 0; r < rounds; r++)
            for (uint32_t t = 0; t < threads; t++) {
                uint32_t row = 0, col = 0;
                if (!rk_tile_tri_cell(r * threads + t, row, col)) continue;
                if (hit[col * 32 + row]++) fail("a cell in two rounds", r * threads + t);
                n_hit++;
            }
        if (n_hit != kTileTriCells) fail("cells of all rounds", threads);
        printf("rounds %u %u %u\n", threads, rounds, n_hit);
    }
    // ---- banks: a 4-byte LDS read is served in groups of 32 lanes, the bank of cnt[col * 32 + row] is its row
    uint32_t worst = 0;
    for (uint32_t g = 0; g < 1024 / 32; g++) {
        uint32_t per_bank[32] = {0};
        for (uint32_t l = 0; l < 32; l++) {
            uint32_t row = 0, col = 0;
            if (rk_tile_tri_cell(g * 32 + l, row, col)) per_bank[(col * 32 + row) % 32]++;
        }
        for (uint32_t b = 0; b < 32; b++)
            if (per_bank[b] > worst) worst = per_bank[b];
    }
    printf("banks %u\n", worst);
    if (worst > 2) fail("reads of one bank in a group of 32 lanes", worst);
    printf("tile_cells_check: ok\n");
    return 0;
}
