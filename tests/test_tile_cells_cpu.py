"""rk_tile_cells.h (the numbering of a diagonal tile's 496 reportable cells in rk_tile_kernel) as plain C++:
tools/tile_cells_check.cpp, compiled here with g++ under -fsanitize=address,undefined, checks the map itself and prints every
number's answer; the properties are checked again here from that print-out.  No GPU call is made."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = 496


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_cells") / "tile_cells_check")
    # (the runtimes are linked statically: the program then needs nothing of the order in which shared libraries are loaded)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"), os.path.join(ROOT, "tools", "tile_cells_check.cpp"), "-o", exe])
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    p = subprocess.run([exe], capture_output=True, text=True, env=e)
    assert p.returncode == 0, (p.stdout[-2000:] + p.stderr)[-4000:]
    assert not any(m in p.stderr for m in ("AddressSanitizer", "runtime error", "LeakSanitizer")), p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "tile_cells_check: ok"
    return out


@pytest.fixture(scope="module")
def cells(lines):
    """{number: (accepted, row, col)} for 0 .. 1023"""
    got = {}
    for l in lines:
        if l.startswith("cell "):
            i, ok, row, col = (int(x) for x in l.split()[1:])
            got[i] = (ok == 1, row, col)
    assert sorted(got) == list(range(1024))
    return got


def test_the_map_is_a_bijection_onto_the_cells_above_the_diagonal(cells):
    image = [cells[i][1:] for i in range(CELLS)]
    assert all(cells[i][0] for i in range(CELLS))
    assert sorted(image) == [(row, col) for row in range(32) for col in range(row + 1, 32)]     # each once, nothing else
    for corner in ((0, 1), (0, 31), (30, 31), (15, 16)):
        assert corner in image


def test_numbers_from_496_on_are_rejected_and_write_nothing(cells):
    for i in range(CELLS, 1024):
        assert cells[i] == (False, 0xDEAD, 0xDEAD), i


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_the_rounds_cover_every_cell_exactly_once(cells, lines, threads):
    rounds = -(-CELLS // threads)
    assert rounds == (2 if threads == 256 else 1)
    held = [cells[r * threads + t][1:] for r in range(rounds) for t in range(threads) if cells[r * threads + t][0]]
    assert len(held) == len(set(held)) == CELLS
    assert "rounds %d %d %d" % (threads, rounds, CELLS) in lines


def test_a_group_of_32_lanes_reads_no_bank_more_than_twice(cells, lines):
    """cnt[col * 32 + row] is read 4 bytes per lane: served in groups of 32 lanes over 32 banks, the bank of a cell is its row"""
    worst = 0
    for g in range(1024 // 32):
        banks = [(col * 32 + row) % 32 for ok, row, col in (cells[g * 32 + l] for l in range(32)) if ok]
        worst = max([worst] + [banks.count(b) for b in set(banks)])
    assert worst == 2 and "banks 2" in lines
