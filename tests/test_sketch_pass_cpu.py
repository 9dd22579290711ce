"""rk_sketch_pass.h (the host arithmetic of a sketch pass) as plain C++: tools/sketch_pass_check.cpp, compiled here with g++, prints
the chunk length, the plan or refusal of a pass with its rows, the grid, the work buffer's layout, the candidate regions of an attempt
and the retry outcome.  Every line is compared with the statements rk_sketch_packed_dev_ex had inline before the header, rewritten
below in the order they stood there -- not with numbers recorded from the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
RANGE, PADDING, BLOCKS, CEILING = 1, 2, 3, 4   # PassRule
CUS = (1, 8, 256, 304)
MAX_BLOCKS = 0x7FFFFFFF
WANT_MAX = ((0xFFFFFFF0 - 192) // 2) << 4


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sketch_pass") / "sketch_pass_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"), os.path.join(ROOT, "tools", "sketch_pass_check.cpp"), "-o", exe])
    return subprocess.check_output([exe], text=True).splitlines()


def error_codes():
    """RK_ERR_ARG and RK_ERR_UNSUPPORTED as the public header defines them"""
    import re
    text = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    return tuple(int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, text).group(1)) for name in ("RK_ERR_ARG", "RK_ERR_UNSUPPORTED"))


# ------------------------------------------------------------------------------------------ the parent's statements, by hand
def chunk_blocks(total_blocks, n_genomes, num_cu, env):
    """env: the value of RK_SKETCH_CB, None when it is not set"""
    wave_slots = num_cu * 2 * 16
    limit = 2 * wave_slots
    if n_genomes < limit:
        cb = (total_blocks + (limit - n_genomes) - 1) // (limit - n_genomes)
    else:
        cb = (total_blocks + limit - 1) // limit
    cb = min(1 << 20, max(16, cb))
    if env is not None:
        cb = min(1 << 20, max(1, env))
    return cb


def grid_and_groups(n_chunks, num_cu, img):
    if not n_chunks:
        return 0, 0   # nothing is launched: the record keeps its zeros
    want = (n_chunks + 15) // 16
    grid = min(want, num_cu * (2 if img else 1))
    n_groups = max(1, min(grid // 16, 32))
    if n_groups > 1:
        grid -= grid % (8 * n_groups)
    return grid, n_groups


def pass_table(genomes, packed_bytes, drlevel, num_cu, img, env):
    """("refused", code, rule, genome) or (cb, n_chunks, grid, n_groups, rows)"""
    total_blocks = 0
    for g, (beg, end) in enumerate(genomes):
        if end < beg or (beg & 1023) or end > packed_bytes:
            return "refused", RK_ERR_ARG, RANGE, g
        if ((end + 1023) & ~1023) > packed_bytes and end > beg:
            return "refused", RK_ERR_ARG, PADDING, g
        if ((end - beg + 1023) >> 10) > 0x7FFFFFFF:
            return "refused", RK_ERR_UNSUPPORTED, BLOCKS, g
        total_blocks += (end - beg + 1023) >> 10
    cb = chunk_blocks(total_blocks, len(genomes), num_cu, env)
    rows, n_chunks = [], 0
    for g, (beg, end) in enumerate(genomes):
        nblk = (end - beg + 1023) >> 10
        first_chunk = n_chunks
        n_chunks += (nblk + cb - 1) // cb
        want = 2 * ((end - beg) >> (4 * drlevel)) + 192
        if want > 0xFFFFFFF0 or n_chunks > 0xFFFFFFF0:
            return "refused", RK_ERR_UNSUPPORTED, CEILING, g
        rows.append((beg, nblk, first_chunk, want))
    rows.append((0, 0, n_chunks, 0))
    return (cb, n_chunks) + grid_and_groups(n_chunks, num_cu, img) + (rows,)


def buffer_layout(n):
    tail_bytes = 16   # SketchTail: two 64-bit words
    res_bytes = tail_bytes + (n + 1) * 8 + n * 4           # tail | off | gcount
    tickets_off = (res_bytes + n * 4 + 127) & ~127
    work_bytes = tickets_off + 32 * 32 * 4
    d_off_copy = tail_bytes
    d_gcount = tail_bytes + (n + 1) * 8
    d_usize = d_gcount + 4 * n                              # d_gcount + n_genomes, a uint32_t pointer
    return 0, d_off_copy, d_gcount, d_usize, tickets_off, res_bytes, work_bytes


def regions(caps, key_bytes):
    total_cap, small_lds, any_big, n_big, max_reg_cap, rows = 0, key_bytes, 0, 0, 0, []
    for cap in caps:
        reg_off = total_cap
        total_cap += cap
        p2 = 1
        while p2 < cap:
            p2 <<= 1
        is_big = int(p2 * key_bytes > 64 * 1024)
        max_reg_cap = max(max_reg_cap, cap)
        if is_big:
            any_big, n_big = 1, n_big + 1
        else:
            small_lds = max(small_lds, p2 * key_bytes)
        rows.append((reg_off, is_big))
    return total_cap, small_lds, n_big, max_reg_cap, any_big, rows


def retry(caps, counts, flag):
    overflow, caps = bool(flag), list(caps)
    max_candidates = max(counts, default=0)
    for g, n in enumerate(counts):
        if n > caps[g]:
            overflow = True
            caps[g] = n
    return int(overflow), max_candidates, caps


# ------------------------------------------------------------------------------------------ the cases of the program
def back_to_back(lengths):
    out, at = [], 0
    for b in lengths:
        out.append((at, at + b))
        at = (at + b + 1023) & ~1023
    return out, at


def plan_lines(name, genomes, packed_bytes, drlevel, num_cu, img, env):
    got = pass_table(genomes, packed_bytes, drlevel, num_cu, img, env)
    if got[0] == "refused":
        return ["plan %s : refused %d %d %d" % ((name,) + got[1:])]
    out = ["plan %s : %d %d %d %d" % ((name,) + got[:4])]
    return out + ["row %s %d : %d %d %d %d" % ((name, g) + row) for g, row in enumerate(got[4])]


def layout_line(name, caps, key_bytes):
    r = regions(caps, key_bytes)
    return " | ".join(["lay %s %d : %d %d %d %d %d" % ((name, key_bytes) + r[:5])] + ["%d %d" % row for row in r[5]])


def retry_lines(name, caps, counts, flag, key_bytes):
    again, most, caps2 = retry(caps, counts, flag)
    return [" ".join(["retry %s : %d %d" % (name, again, most)] + [str(c) for c in caps2]), layout_line(name, caps2, key_bytes)]


def expected():
    out = []
    for cu in CUS:
        limit = 4 * 16 * cu
        for n in (limit - 1, limit, limit + 1):
            d = limit - n if n < limit else limit
            for total in (0, 1, 15 * d, 16 * d, 16 * d + 1, d << 20, (d << 20) + 1):
                out.append("cb %d %d %d 0 : %d" % (cu, n, total, chunk_blocks(total, n, cu, None)))
    for v in (0, 1, 3, (1 << 20) + 1):
        out.append("cb 8 4 1000 %d : %d" % (v, chunk_blocks(1000, 4, 8, v)))
    n_chunk_length = len(out)

    for name, lengths, dr, cu, img, env in (("sizes", [0, 1, 1024, 1025], 3, 8, 1, None), ("cb3", [3 * 1024, 4 * 1024, 3 * 1024 + 1], 3, 8, 1, 3),
                                            ("gaps", [0, 5 * 1024, 0, 0, 2 * 1024 + 1, 0], 3, 8, 1, 2), ("none", [], 3, 8, 1, None),
                                            ("empty3", [0, 0, 0], 3, 8, 1, None)):
        out += plan_lines(name, *back_to_back(lengths), dr, cu, img, env)
    for dr in (1, 2, 3, 4):
        out += plan_lines("dr%d" % dr, *back_to_back([1000000, 70000]), dr, 304, 2, None)
    M = MAX_BLOCKS
    for name, genomes, packed_bytes, dr, env in (
            ("end_before_beg", [(0, 1024), (2048, 2047)], 4096, 3, None),
            ("beg_unaligned", [(0, 1024), (1025, 2048)], 4096, 3, None),
            ("end_beyond", [(0, 1024), (1024, 4097)], 4096, 3, None),
            ("tail_unpadded", [(0, 1024), (2048, 2049)], 2049, 3, None),
            ("tail_empty_genome", [(0, 1024), (2048, 2048)], 2049, 3, None),
            ("blocks_at_31_bits", [(0, M << 10)], M << 10, 4, None),
            ("blocks_beyond_31_bits", [(0, (M << 10) + 1)], (M + 1) << 10, 4, None),
            ("region_at_ceiling", [(0, WANT_MAX)], (WANT_MAX + 1023) & ~1023, 1, None),
            ("region_beyond_ceiling", [(1024, 1024 + WANT_MAX + 16)], (1024 + WANT_MAX + 16 + 1023) & ~1023, 1, None),
            ("chunks_beyond_ceiling", [(0, M << 10), (M << 10, 2 * M << 10), (2 * M << 10, 3 * M << 10)], 3 * M << 10, 4, 1),
            ("range_before_region", [(0, WANT_MAX + 16), (5, 6)], (WANT_MAX + 16 + 1023) & ~1023, 1, None)):
        out += plan_lines(name, genomes, packed_bytes, dr, 8, 1, env)
    n_plan = len([l for l in out if l.startswith("plan ")])

    for cu in CUS:
        for img in (0, 1, 2):
            for chunks in (0, 1, 16, 17, 32 * cu, 32 * cu + 1, 496, 512, 640, 9600):
                out.append("grid %d %d %d : %d %d" % ((cu, img, chunks) + grid_and_groups(chunks, cu, img)))
    for n in (0, 1, 31, 32):
        out.append("buf %d : %d %d %d %d %d %d %d" % ((n,) + buffer_layout(n)))
    for name, caps, key_bytes in (("k4", [16384, 16385, 192], 4), ("k8", [8192, 8193, 100], 8), ("big_only", [16385], 4), ("big_only", [8193, 8193], 8),
                                  ("none", [], 4), ("mixed", [192, 5000, 0, 1, 4097], 4), ("mixed", [192, 5000, 0, 1, 4097], 8)):
        out.append(layout_line(name, caps, key_bytes))
    for name, caps, counts, flag, key_bytes in (("fits", [192, 1000], [192, 7], 0, 4), ("flag_alone", [192, 1000], [10, 20], 1, 4),
                                                ("one_above", [192, 1000, 300], [10, 1001, 300], 0, 4), ("turns_big", [192, 1000], [10, 20000], 1, 4),
                                                ("turns_big", [192, 1000], [10, 8193], 1, 8), ("none", [], [], 0, 4)):
        out += retry_lines(name, caps, counts, flag, key_bytes)
    return out, n_chunk_length, n_plan


def test_error_codes_are_the_public_ones():
    assert error_codes() == (RK_ERR_ARG, RK_ERR_UNSUPPORTED)


def test_every_line_equals_the_rules_it_replaces(lines):
    want, n_chunk_length, n_plan = expected()
    for mine, theirs in zip(lines, want):
        assert mine == theirs
    kinds = {k: sum(1 for l in lines if l.startswith(k + " ")) for k in ("cb", "plan", "row", "grid", "buf", "lay", "retry")}
    assert len(lines) == len(want) == sum(kinds.values())
    assert (n_chunk_length, n_plan) == (88, 20)
    assert kinds == {"cb": 88, "plan": 20, "row": 40, "grid": 120, "buf": 4, "lay": 13, "retry": 6}


def test_the_cases_reach_their_edges(lines):
    """conditions on the cases themselves: that each one stands where the issue's list puts it"""
    got = {l.split(" : ")[0]: l.split(" : ")[1] for l in lines}
    # chunk length: both sides of the clamp at 16, the one at 2^20, both branches of the rule, the override's clamps
    for cu in CUS:
        limit = 64 * cu
        for n in (limit - 1, limit, limit + 1):
            d = limit - n if n < limit else limit
            assert [got["cb %d %d %d 0" % (cu, n, t)] for t in (0, 1, 15 * d, 16 * d, 16 * d + 1, d << 20, (d << 20) + 1)] == \
                ["16", "16", "16", "16", "17", str(1 << 20), str(1 << 20)]
    assert [got["cb 8 4 1000 %d" % v] for v in (0, 1, 3, (1 << 20) + 1)] == ["1", "1", "3", str(1 << 20)]
    # rows: 0 bytes no chunk and 192 slots; 1, 1,024 and 1,025 bytes one, one and two blocks
    assert [got["row sizes %d" % g].split()[1:] for g in range(5)] == [["0", "0", "192"], ["1", "0", "192"], ["1", "1", "192"], ["2", "2", "192"], ["0", "3", "0"]]
    assert [got["row cb3 %d" % g].split()[2] for g in range(4)] == ["0", "1", "3", "5"]          # cb blocks one chunk, cb + 1 two
    assert [got["row gaps %d" % g].split()[2] for g in range(7)] == ["0", "0", "3", "3", "3", "5", "5"]   # empty genomes share their successor's first chunk
    assert got["plan none"] == got["plan empty3"] == "16 0 0 0"
    assert [got["row dr%d 0" % dr].split()[3] for dr in (1, 2, 3, 4)] == [str(2 * (1000000 >> 4 * dr) + 192) for dr in (1, 2, 3, 4)]
    # refusals: code, rule, genome
    want = {"end_before_beg": (RK_ERR_ARG, RANGE, 1), "beg_unaligned": (RK_ERR_ARG, RANGE, 1), "end_beyond": (RK_ERR_ARG, RANGE, 1),
            "tail_unpadded": (RK_ERR_ARG, PADDING, 1), "blocks_beyond_31_bits": (RK_ERR_UNSUPPORTED, BLOCKS, 0),
            "region_beyond_ceiling": (RK_ERR_UNSUPPORTED, CEILING, 0), "chunks_beyond_ceiling": (RK_ERR_UNSUPPORTED, CEILING, 1),
            "range_before_region": (RK_ERR_ARG, RANGE, 1)}
    for name, what in want.items():
        assert got["plan " + name] == "refused %d %d %d" % what, name
    for name in ("tail_empty_genome", "blocks_at_31_bits", "region_at_ceiling"):
        assert not got["plan " + name].startswith("refused"), name
    assert got["row region_at_ceiling 0"].split()[3] == str(0xFFFFFFF0)
    # grid: 1, 2 and 32 groups, grids that the rounding shortens, nothing to scan
    assert got["grid 256 1 496"] == "31 1" and got["grid 256 1 640"] == "32 2" and got["grid 256 1 9600"] == "512 32"
    assert got["grid 304 1 %d" % (32 * 304 + 1)] == "512 32" and got["grid 304 0 9600"] == "304 19" and got["grid 8 2 0"] == "0 0"
    # the work buffer: tickets at a 128-byte boundary behind the sizes
    for n in (0, 1, 31, 32):
        tail, off, gcount, usize, tickets, res_bytes, work_bytes = (int(x) for x in got["buf %d" % n].split())
        assert tickets % 128 == 0 and tickets >= res_bytes + 4 * n and usize == res_bytes and work_bytes == tickets + 4096
    # regions: the LDS sort's last capacity and the first beyond, per key width; no small genome: one key of LDS
    assert got["lay k4 4"] == "32961 65536 1 16385 1 | 0 0 | 16384 1 | 32769 0"
    assert got["lay k8 8"] == "16485 65536 1 8193 1 | 0 0 | 8192 1 | 16385 0"
    assert got["lay big_only 4"].startswith("16385 4 1 ") and got["lay big_only 8"].startswith("16386 8 2 ") and got["lay none 4"] == "0 4 0 0 0"
