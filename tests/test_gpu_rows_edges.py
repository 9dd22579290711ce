"""rk_dist_kernel (rabbitkssd_amd/csrc/rk_dist.hip), the self join with full counter rows, at its slice, pair and
list edges, against the oracle (ok.index_build32 / ok.index_dist32; the 64-bit pair once).  Integers equal, jorc and dist bit
for bit.

An equal result proves nothing about an edge unless the edge was taken, so every leg asserts, in this order: the seam from the
model of tests/_rows_ref.py (the same conditions tests/test_rows_ref_cpu.py checks without a GPU), the kernel variant
(rk_dist_kernel_name), the plan's `band:` lines where tiles matter (RK_DIST_DEBUG=1), rk_index_self_stats against the model's
slice totals, and then the hits.

    seam                                                        leg
    compact lists on the window's last column, rotated walk     test_slice_forms (hub row 10)
    ranges of 2 .. 8 | 9 .. 24 | 25 .. 24 + 129 postings        test_slice_forms
    four 16-lane rows, a fifth and sixth long list in a wave,   test_slice_forms (first wave, last wave of a batch, second batch at
      in every batch position                                     256 / 512 / 1,024 threads)
    multiset sketches: ranges only, 32-bit counters             test_slice_forms[multiset]
    pair sharing: the partner itself, shared / open / covered   test_slice_forms (the pair 40, 41), self_stats[2]
    lone last row, empty sketches in a pair, odd row blocks     test_slice_forms, test_row_shards
    per-unit list at cap - 1, cap, cap + 1; unit after overflow test_per_unit_list
    batch lists: flush at cap / 2, overflow, exactly cap, final test_batch_lists
    the lists under column tiles (rows zeroed per unit)         test_lists_under_column_tiles
    16-bit counters at 65,535, 32-bit from 65,536 / repeats     test_counter_width
    rk_dist_rows_dev over its capacity                          test_device_hits_over_capacity
    the persistent per-XCD queues, the stage's per-hit path     test_persistent_queues
    list mode (rk_near_kernel's fallback) under column tiles    test_fallback_list_under_column_tiles
    bands: col_base left of a band's first row, pairs across    test_bands
      band and tile boundaries, boundaries in row shards

Developer switches are read when a context is created: every leg makes its own (tests/_gpu_join.py make_ctx)."""
import re

import numpy as np
import pytest

from oracle import oracle as ok

import _gpu_join as gj
import _prune_ref as pr
import _rows_ref as rr
from _gpu_join import assert_hits_equal, make_ctx

pytestmark = pytest.mark.gpu
K = rr.K
ROWS_ONLY = {"RK_DIST_NEAR": "0", "RK_DIST_TILES": "0"}      # the kernels with counter rows, the generator's ids
BAND_LINE = re.compile(r"\[rk\] band: columns from (\d+), units (\d+) from slot (\d+), kernel <(u16|u32), (\d), (\d+)>, (\d+) B LDS, (\d+) tile\(s\)")


def ctx_for(monkeypatch, env):
    return make_ctx(monkeypatch, dict(ROWS_ONLY, **env))


def build(ctx, key):
    h, off, bits = rr.collection(key)[:3]
    idx = ctx.index_build(ctx.sketches_from_host(h, off), bits)
    assert np.array_equal(idx.order, np.arange(len(off) - 1))
    return idx


def join(ctx, idx, metric, D, **shard):
    return gj.join(ctx, idx, metric, D, K, **shard)


def bands_of(capfd):
    """the plan's band lines since the last call: [(columns from, units, slot, counters, mode, threads, tiles)]"""
    return [(int(m[1]), int(m[2]), int(m[3]), m[4], int(m[5]), int(m[6]), int(m[8])) for m in BAND_LINE.finditer(capfd.readouterr().err)]


# ---- A and B: slice forms at their seams, pair sharing ----------------------------------------------------------------------
def forms_name(multiset, pair, threads):
    """make_plan for 337 columns: rows of a few hundred bytes, so 256 threads (512 for pairs) unless forced"""
    paired = pair == "default" and not multiset
    return paired, "rk_dist_kernel<%s, %d, %s>" % ("false" if multiset else "true", 2 if paired else 1, threads or ("512" if paired else "256"))


FORMS_CASES = [(False, pair, threads) for pair in ("default", "2") for threads in (None, "256", "1024")] + \
              [(True, "default", threads) for threads in (None, "256", "1024")]      # (multisets never pair: RK_DIST_PAIR changes nothing)


@pytest.mark.parametrize("multiset,pair,threads", FORMS_CASES,
                         ids=["%s-%s-%s" % ("multiset" if m else "sets", p, t) for m, p, t in FORMS_CASES])
def test_slice_forms(monkeypatch, multiset, pair, threads):
    """The hub row 10 of tests/_rows_ref.py forms_collection owns 1,100 slices placed wave by wave: compact lists with
    (first, last) - base in {0, 1, 30, 31} x {31, 32}, all 32 bits, bit 31 alone, eight rotations side by side; ranges of every
    length at 8 | 9, 24 | 25 and the stream's trips; six long lists in the first wave, the last wave of the first batch and the
    second batch.  The pair (40, 41) shares hashes in every form, each member has open slices of every form, 41 has covered
    ones; 320 and 325 are empty members of pairs; the last row is alone.  Forced 256 threads: pairs without batch lists.  The
    multiset twin (one hash twice in one sketch) has no compact slice and no pairs.  Sparse under a threshold that reports every
    designated cell, and the dense report, which returns every cell's count."""
    paired, name = forms_name(multiset, pair, threads)
    totals = rr.forms_conditions(multiset, paired, int(threads or (512 if paired else 256)))
    key = ("forms", multiset)
    designated = rr.collection(key)[3]
    env = {} if pair == "default" else {"RK_DIST_PAIR": pair}
    if threads:
        env["RK_DIST_THREADS"] = threads
    ctx = ctx_for(monkeypatch, env)
    try:
        idx = build(ctx, key)
        for D in (rr.FORMS_D, 1.5):
            want = rr.oracle_hits(key, 1, D)
            cells = rr.hit_cells(want)
            assert all(cells.get(k) == v for k, v in designated.items())
            assert ctx.dist_kernel_name(idx, None, 1, 1, K, D) == name
            assert idx.self_stats[0:3] == totals
            assert_hits_equal(join(ctx, idx, 1, D), want)
            assert_hits_equal(join(ctx, idx, 1, D), want)
        del idx
    finally:
        ctx.close()


@pytest.mark.parametrize("multiset", [False, True], ids=["sets", "multiset"])
def test_row_shards(monkeypatch, multiset):
    """the same collection in row shards: blocks of 16 and 64 rows keep the pairs, blocks of one row switch them off"""
    key = ("forms", multiset)
    paired, name = forms_name(multiset, "default", None)
    totals = rr.forms_conditions(multiset, paired, 512 if paired else 256)
    ctx = ctx_for(monkeypatch, {})
    try:
        idx = build(ctx, key)
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, rr.FORMS_D, row_first=1, row_step=3, row_block=16) == name
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, rr.FORMS_D, row_first=1, row_step=5, row_block=1) == forms_name(multiset, "2", None)[1]
        assert idx.self_stats[0:3] == totals
        gj.assert_shards(ctx, idx, 1, rr.FORMS_D, K, rr.oracle_hits(key, 1, rr.FORMS_D), ((3, 16), (2, 64), (5, 1)))
        del idx
    finally:
        ctx.close()


# ---- C: the cell list at capacity -----------------------------------------------------------------------------------------------
def cap_env(cap):
    return {} if cap == 256 else {"RK_DIST_CAND_CAP": str(cap)}


def lists_leg(monkeypatch, env, name, totals, capfd=None, tiles=None):
    ctx = ctx_for(monkeypatch, env)
    try:
        idx = build(ctx, ("lists",))
        want = rr.oracle_hits(("lists",), 1, rr.LISTS_D)
        if capfd is not None:
            capfd.readouterr()
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, rr.LISTS_D) == name
        if capfd is not None:
            bands = bands_of(capfd)
            assert len(bands) == 1 and bands[0][0] == 0 and bands[0][6] == tiles and rr.tile_cols_of(rr.LISTS_N, tiles) == 512, bands
        assert idx.self_stats[0:3] == totals
        for _ in range(2):
            assert_hits_equal(join(ctx, idx, 1, rr.LISTS_D), want)      # (lengths first: a pair reported twice fails here)
        if capfd is not None:
            launched = bands_of(capfd)       # (a join whose hits exceed the first buffer launches again with the exact count)
            assert len(launched) >= 2 and all(b[4] == 0 and b[6] == tiles for b in launched), launched
        del idx
    finally:
        ctx.close()


@pytest.mark.parametrize("cap", rr.LISTS_CAPS)
def test_per_unit_list(monkeypatch, cap):
    """Single rows, 256 threads, two consecutive rows per workgroup, rows kept clean: rows with cap - 4 .. cap + 9 cells and one
    well above, each followed by a row of three cells -- its rows must be clean again after the overflow walk, and its counter is
    the other one of the pair.  The targets start off a quad boundary, so the quad at the list's end fits partly."""
    totals = rr.lists_conditions(cap, "single")
    env = dict(cap_env(cap), RK_DIST_PAIR="2", RK_DIST_THREADS="256", RK_DIST_PERSIST="2", RK_DIST_ROWS="2")
    lists_leg(monkeypatch, env, "rk_dist_kernel<true, 1, 256>", totals)


@pytest.mark.parametrize("threads", ["512", "1024"])
@pytest.mark.parametrize("cap", rr.LISTS_CAPS)
def test_batch_lists(monkeypatch, cap, threads):
    """Row pairs, four known consecutive units per workgroup (RK_DIST_PERSIST=2 RK_DIST_ROWS=4): the model's runs hold a flush
    at exactly cap / 2, cap / 2 - 1 waiting entries and a unit that makes cap + 1, a unit alone above cap, a fill to exactly cap
    and entries still waiting at the end of a run."""
    totals = rr.lists_conditions(cap, "pairs")
    env = dict(cap_env(cap), RK_DIST_PERSIST="2", RK_DIST_ROWS="4")
    if threads != "512":
        env["RK_DIST_THREADS"] = threads
    lists_leg(monkeypatch, env, "rk_dist_kernel<true, 2, %s>" % threads, totals)


@pytest.mark.parametrize("threads", ["256", "512"])
@pytest.mark.parametrize("cap", rr.LISTS_CAPS)
def test_lists_under_column_tiles(monkeypatch, capfd, cap, threads):
    """The same rows with an LDS row of 512 columns (RK_DIST_LDS_KB=1; plan_bands leaves 1,001 rows in one band, whose
    line says two tiles): two column tiles, range-checked postings, rows
    zeroed per unit and NOT kept clean.  Rows bring more than cap cells into one tile, and the targets of some lie on both sides
    of column 512.  A unit over the list's capacity must not report the cells that fitted twice: once from the list and once
    from the walk over the rows."""
    totals = rr.lists_conditions(cap, "tiles", 512)
    env = dict(cap_env(cap), RK_DIST_LDS_KB="1", RK_DIST_THREADS=threads, RK_DIST_DEBUG="1")
    lists_leg(monkeypatch, env, "rk_dist_kernel<true, 0, %s>" % threads, totals, capfd, 2)


# ---- E: counter width -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big,repeat,name", [(65535, False, "rk_dist_kernel<true, 2, 512>"), (65536, False, "rk_dist_kernel<false, 2, 512>"),
                                             (65535, True, "rk_dist_kernel<false, 1, 256>")])
def test_counter_width(monkeypatch, big, repeat, name):
    """Three identical sketches of 65,535 hashes: the largest count two 16-bit counters of a word can hold, in the high half
    (6, 9) and in the low half (6, 12), (9, 12), with non-zero neighbours in the other halves.  One hash more, or one hash twice
    in a sketch, and the counters are 32 bits wide."""
    key = ("width", big, repeat)
    h, off, _ = rr.collection(key)
    a, b, c = rr.WIDTH_BIG
    ctx = ctx_for(monkeypatch, {})
    try:
        idx = build(ctx, key)
        for D in (0.1, 1.5):
            want = rr.oracle_hits(key, 1, D)
            cells = rr.hit_cells(want)
            assert cells[(a, c)] == big and cells[(a, b)] == big + repeat and cells[(a, b - 1)] == 3 and cells[(a, c + 1)] == 3
            assert ctx.dist_kernel_name(idx, None, 1, 1, K, D) == name
            assert idx.self_stats[0:3] == rr.slice_totals(rr.slices(h, off))
            assert_hits_equal(join(ctx, idx, 1, D), want)
        del idx
    finally:
        ctx.close()


# ---- F: rk_dist_rows_dev over its capacity ------------------------------------------------------------------------------------
F_STAGE = 16          # RK_DIST_STAGE_HITS: hits a workgroup stages; a unit has one workgroup per tile at most
F_LEGS = {
    # switches, threshold, kernel, column tiles
    "sparse": ({}, rr.LISTS_D, "rk_dist_kernel<true, 2, 512>", 1),
    "sparse_tiled": ({"RK_DIST_LDS_KB": "1"}, rr.LISTS_D, "rk_dist_kernel<true, 0, 256>", 2),
    "dense": ({}, 1.5, "rk_dist_kernel<true, 2, 512>", 1),
}


@pytest.mark.parametrize("leg", list(F_LEGS))
def test_device_hits_over_capacity(monkeypatch, capfd, leg):
    """hits_cap at a third of the true count.  Sparse: more hits than all workgroups together can stage (no more workgroups
    than rows, padded to whole XCD chunks, per tile; RK_DIST_STAGE_HITS each), so staged records and records written one by one
    both meet the end of the buffer; dense: the reserved slots.  *n_hits_dev is the oracle's count, the `cap` records are
    distinct members of the result, the guard is untouched."""
    env, D, name, tiles = F_LEGS[leg]
    want = rr.oracle_hits(("lists",), 1, D)
    n = rr.LISTS_N
    assert len(want) > F_STAGE * ((n + 63) // 64 * 64) * tiles and (D < 1 or len(want) == n * (n - 1) // 2)
    ctx = ctx_for(monkeypatch, dict(env, RK_DIST_STAGE_HITS=str(F_STAGE), RK_DIST_DEBUG="1"))
    try:
        idx = build(ctx, ("lists",))
        capfd.readouterr()
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, D) == name
        bands = bands_of(capfd)
        assert len(bands) == 1 and bands[0][6] == tiles, bands
        cap = len(want) // 3
        got_n, got = gj.dev_records(ctx, idx, None, 1, 1, D, K, cap)       # (asserts the guard)
        gj.assert_capped_records(got_n, got, want, cap, n)
        del idx
    finally:
        ctx.close()


def test_device_hits_over_capacity_wide_hashes(monkeypatch):
    """the same through the index of 36-bit hashes (rk_sketches_from_host64), against the oracle's 64-bit pair"""
    h, off, _ = rr.lists_collection()
    h64 = h.astype(np.uint64) << np.uint64(10)
    uhash, ucount, postings = ok.index_build64(h64, off)
    want, _ = ok.index_dist64(uhash, ucount, postings, np.diff(off).astype(np.uint32), h64, off, 1, 1, K, rr.LISTS_D, threads=8)
    assert_hits_equal(want, rr.oracle_hits(("lists",), 1, rr.LISTS_D))      # (the same sets under wider names)
    ctx = ctx_for(monkeypatch, {})
    try:
        idx = ctx.index_build(ctx.sketches_from_host64(h64, off), 36)
        assert np.array_equal(idx.order, np.arange(len(off) - 1))
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, rr.LISTS_D) == "rk_dist_kernel<true, 2, 512>"
        assert idx.self_stats[0:3] == rr.lists_conditions(256, "pairs")
        assert_hits_equal(join(ctx, idx, 1, rr.LISTS_D), want)
        cap = len(want) // 3
        got_n, got = gj.dev_records(ctx, idx, None, 1, 1, rr.LISTS_D, K, cap)
        gj.assert_capped_records(got_n, got, want, cap, rr.LISTS_N)
        del idx
    finally:
        ctx.close()


# ---- C3: more units than the chip holds workgroups: the persistent per-XCD queues ---------------------------------------------
def test_persistent_queues(monkeypatch):
    """1,100 pairs, heavy (more cells than the list holds), light and empty rows in random order, 24 staged hits per workgroup:
    the grid of one workgroup per unit exceeds what the chip can hold at once -- at most four workgroups of eight waves per CU
    (32 wave slots), and no more than the LDS of a CU over a workgroup's footprint in granules of 1,280 bytes -- so the launch is
    persistent and every workgroup walks its XCD's queue; and the hits exceed what all workgroups can stage."""
    import torch
    stage = 24
    grid, totals = rr.queues_conditions(stage)
    n = rr.QUEUES_N
    row_bytes = (((n + 1) // 2 + 3) & ~3) * 4                       # one 16-bit counter row in whole 16-byte quads
    footprint = 2 * row_bytes + 256 * 8 + stage * gj.REC + 64 + (2 * 256 * 16 - 256 * 8)    # rows, list, stage, scalars, batch lists
    per_cu = min(32 // (512 // 64), (160 * 1024) // ((footprint + 1279) // 1280 * 1280))
    assert grid > per_cu * torch.cuda.get_device_properties(0).multi_processor_count, (grid, per_cu)
    ctx = ctx_for(monkeypatch, {"RK_DIST_STAGE_HITS": str(stage)})
    try:
        idx = build(ctx, ("queues",))
        want = rr.oracle_hits(("queues",), 1, rr.LISTS_D)
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, rr.LISTS_D) == "rk_dist_kernel<true, 2, 512>"
        assert idx.self_stats[0:3] == totals
        for _ in range(2):
            assert_hits_equal(join(ctx, idx, 1, rr.LISTS_D), want)
        del idx
    finally:
        ctx.close()


# ---- C5: list mode (the fallback launch of rk_near_kernel) under column tiles --------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_fallback_list_under_column_tiles(monkeypatch, metric):
    """The loud sites of tests/_prune_ref.py and a far family -- 20 genomes behind the window with first_reportable hashes of
    their row -- under the near-window kernel with an LDS row of 512 columns and a cell list of 16 entries: the family's row
    falls back, the fallback launch (list mode, single rows) runs in two column tiles, and the row brings more cells into one
    tile than the list holds.  Three joins: the second resets the list, the third may skip an empty launch."""
    key = ("sites", "family", metric)
    h, off, _ = pr.collection(key)
    D, mrs = pr.SITE_D[metric], pr.site_min_ref_size("family", metric)
    n = len(off) - 1
    sizes = np.diff(off).astype(np.int64)
    assert sizes.min() == mrs and rr.tile_cols_of(n, 2) < n <= 2 * 512
    fb = pr.falls_back(h, off, metric, D, mrs, True)
    cells = rr.candidates(rr.common_matrix(h, off), sizes, metric, D, tile_cols=rr.tile_cols_of(n, 2))
    assert fb and any(cells[r].max() > 16 for r in fb), fb
    ctx = make_ctx(monkeypatch, {"RK_DIST_TILES": "0", "RK_DIST_LDS_KB": "1", "RK_DIST_CAND_CAP": "16"})
    try:
        idx = ctx.index_build(ctx.sketches_from_host(h, off), pr.BITS)
        assert np.array_equal(idx.order, np.arange(n))
        want = pr.oracle_hits(key, metric, D)
        assert ctx.dist_kernel_name(idx, None, 1, metric, K, D).startswith("rk_near_kernel<true, ")
        for _ in range(3):
            assert_hits_equal(join(ctx, idx, metric, D), want)
        assert ctx.dist_kernel_name(idx, None, 1, metric, K, D).startswith("rk_near_kernel<true, ")
        del idx
    finally:
        ctx.close()


# ---- D: bands ---------------------------------------------------------------------------------------------------------------------
BANDS_N = 2999
BANDS_ENV = {"RK_DIST_BAND_MIN_ROWS": "64", "RK_DIST_LDS_KB": "16", "RK_DIST_DEBUG": "1"}


def band_rows(bands, step=1, block=1):
    """first row of every band: its first unit slot times the rows of a unit, in rounds of step * block rows"""
    return [b[2] * (2 if b[4] == 2 else 1) * step for b in bands]


@pytest.mark.parametrize("shard", [None, (3, 16), (2, 64)], ids=["all", "3x16", "2x64"])
def test_bands(monkeypatch, capfd, shard):
    """2,999 short sketches under an LDS of 16 KiB and bands of at least 64 rows.  The plan depends on the size of the
    collection alone, so the test reads it first -- the `band:` lines of an index of 2,999 unrelated sketches -- and then builds
    the collection around it: relatives on either side of every band boundary, both ways for the rows of a pair, and for a row
    of every tiled band its cells on the last column of a tile and the first of the next.  The first band is tiled, the last is
    not, and the variant changes at every boundary.  In row shards a boundary lies on a multiple of row_step * row_block: with
    rounds of 48 rows some band starts on a row that is no multiple of 64, and its LDS rows begin to the left of it
    (col_base = row & ~63)."""
    step, block = shard or (1, 0)
    opts = dict(row_first=0, row_step=step, row_block=block) if shard else {}
    ctx = ctx_for(monkeypatch, BANDS_ENV)
    try:
        plain = rr.bands_collection(BANDS_N, [])
        probe = ctx.index_build(ctx.sketches_from_host(plain[0], plain[1]), plain[2])
        capfd.readouterr()
        name = ctx.dist_kernel_name(probe, None, 1, 1, K, rr.BANDS_D, **opts)
        bands = bands_of(capfd)
        del probe
        assert len(bands) >= 2 and name.endswith("[%d bands]" % len(bands)), (name, bands)
        assert bands[0][4] == 0 and bands[0][6] > 1 and bands[-1][6] == 1, bands              # tiled first, one tile last
        assert all(x[4:7] != y[4:7] for x, y in zip(bands, bands[1:])), bands                 # a boundary where the variant changes
        rows_per_unit = [2 if b[4] == 2 else 1 for b in bands]
        if shard:
            # slot -> row of shard 0: blocks of `block` rows, a round of step * block rows apart
            first = [(b[2] * u // block) * step * block for b, u in zip(bands, rows_per_unit)]
            assert all(f % (step * block) == 0 for f in first)
            assert step * block % 64 == 0 or any(f % 64 != 0 for f in first[1:]), first        # col_base lies left of the band's first row
        else:
            first = [b[2] * u for b, u in zip(bands, rows_per_unit)]
        assert all(b[0] == f & ~63 for b, f in zip(bands, first)), (bands, first)
        edges = []
        for b, f in zip(bands, first):
            tile = rr.tile_cols_of(BANDS_N - b[0], b[6])
            edges += [(f, b[0] + k * tile) for k in range(1, b[6])]
        pairs = rr.bands_pairs(BANDS_N, first[1:], edges)
        assert len(pairs) >= 4 * (len(bands) - 1) + 2 * len(edges) and edges
        h, off, bits = rr.bands_collection(BANDS_N, pairs)
        want = rr.dist_hits(h, off, bits, 1, rr.BANDS_D)
        assert gj.pairs_of(want) == set(pairs)                        # every designed pair is reportable, nothing else is
        idx = ctx.index_build(ctx.sketches_from_host(h, off), bits)
        assert np.array_equal(idx.order, np.arange(BANDS_N))
        capfd.readouterr()
        assert ctx.dist_kernel_name(idx, None, 1, 1, K, rr.BANDS_D, **opts) == name
        assert bands_of(capfd) == bands
        assert idx.self_stats[0:3] == rr.slice_totals(rr.slices(h, off))
        if shard:
            gj.assert_shards(ctx, idx, 1, rr.BANDS_D, K, want, (shard,))
        else:
            assert_hits_equal(join(ctx, idx, 1, rr.BANDS_D), want)
            launched = bands_of(capfd)
            assert launched[:len(bands)] == bands, launched
        del idx
    finally:
        ctx.close()
