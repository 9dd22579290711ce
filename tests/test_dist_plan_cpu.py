"""rk_dist_plan.h (host arithmetic shared by the distance joins) as plain C++: tools/dist_plan_check.cpp, compiled here with
g++, prints RowShard's counts and rk_min_jorc; the expected values come from the two counting loops that rk_dist_rows and
rk_cluster_rows had before the header, rewritten below, and from the threshold's expression evaluated with math.exp."""
import math
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dist_plan") / "dist_plan_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"), os.path.join(ROOT, "tools", "dist_plan_check.cpp"), "-o", exe])
    return subprocess.check_output([exe], text=True).splitlines()


def shard(n, step, first, block, all_rows):
    row_step = step if step else 1
    row_block = block if block > 0 else 1
    if all_rows and row_step == 1 and first == 0:
        row_block = all_rows
    return row_step, row_block


def rows_as_rk_dist_rows(n, step, first, block, all_rows):
    """(rows, blocks) of the shard: the loop of rk_dist_rows, one step per row"""
    row_step, row_block = shard(n, step, first, block, all_rows)
    n_sel = n_blk = 0
    blk = first
    while blk * row_block < n:
        n_blk += 1
        for _ in range(blk * row_block, min(n, (blk + 1) * row_block)):
            n_sel += 1
        blk += row_step
    return n_sel, n_blk


def rows_as_rk_cluster_rows(n, step, first, block, all_rows):
    """the loop of rk_cluster_rows, one step per block"""
    row_step, row_block = shard(n, step, first, block, all_rows)
    n_sel = 0
    blk = first
    while blk * row_block < n:
        n_sel += min(n, (blk + 1) * row_block) - blk * row_block
        blk += row_step
    return n_sel


def test_row_shard_counts_equal_the_loops_they_replace(lines):
    got = {}
    for l in lines:
        if l.startswith("rows "):
            key, val = l[5:].split(" : ")
            got[tuple(int(x) for x in key.split())] = tuple(int(x) for x in val.split())
    cases = 0
    for n in (0, 1, 15, 16, 17, 1000):
        for step in (0, 1, 2, 3, 8):
            for first in sorted({0, 1, step - 1, step} - {-1}):
                for block in (0, 1, 2, 16):
                    for all_rows in sorted({0, 16, n}):
                        n_sel, n_blk = rows_as_rk_dist_rows(n, step, first, block, all_rows)
                        assert rows_as_rk_cluster_rows(n, step, first, block, all_rows) == n_sel
                        assert got[(n, step, first, block, all_rows)] == (n_sel, n_blk, max(1 << 16, n_sel * 64)), (n, step, first, block, all_rows)
                        cases += 1
    assert cases == len(got) == 960
    assert got[(1000, 3, 2, 16, 0)][:2] == (328, 21) and got[(1000, 1, 0, 0, 1000)][:2] == (1000, 1)   # (a shard that owns the short last block; all rows as one block)


def float_key(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def test_min_jorc_is_the_expression_it_replaces(lines):
    got = {}
    for l in lines:
        if l.startswith("jorc "):
            key, val = l[5:].split(" : ")
            k, d, metric = key.split()
            got[(int(k), float.fromhex(d), int(metric))] = float.fromhex(val)
    assert len(got) == 12
    for k in (10, 21):
        for D in (0.05, 0.3, 1.0):
            for metric in (0, 1):
                t = math.exp(-float(k) * D)
                want = (t if metric else t / (2.0 - t)) * (1.0 - 1e-6)
                mine = got[(k, D, metric)]
                assert 0.0 < mine < 1.0 and abs(float_key(mine) - float_key(want)) <= 1, (k, D, metric, mine.hex(), want.hex())
