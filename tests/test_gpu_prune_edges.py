"""The pruning bounds of the self join at equality, in all three kernels, against the oracle (ok.index_build32 / ok.index_dist32).

Every kernel skips what cannot hold a reportable pair -- common >= min_jorc * (a lower bound of the denominator) -- and a prune
that is too eager loses hits without a sign.  The collections of tests/_prune_ref.py put pairs ON those bounds (hashes disjoint
by construction, RK_INDEX_RELABEL=0 so that the generator decides blocks and windows), and its model says what the device must
show besides the oracle's hits:

    model                                   device observable
    tiles(): tile count, record count       rk_index_tile_stats [0], [2], from the lazy builder and from the build
    launch_grid()                           rk_index_tile_stats [1] per (metric, D)
    tiles()["lb"], first_reportable         the hits with RK_TILE_ALL=1 (the tile kernel's own `take` test is the only prune)
    falls_back() (far_records, floor_common) rk_dist_kernel_name after completed joins: stays rk_near_kernel / moves to rk_tile_kernel
    floor_common, first_reportable          the hits of rk_near_kernel (window cells) and rk_dist_kernel (candidate list)

The conditions the collections were built for are checked on the CPU (tests/test_prune_ref_cpu.py) and asserted again here.
Developer switches are read when a context is created, RK_TILE_THREADS / RK_TILE_SROW / RK_TILE_ALL at every launch."""
import math

import numpy as np
import pytest

import _gpu_join as gj
import _prune_ref as pr
from _gpu_join import assert_hits_equal, make_ctx, pairs_of

pytestmark = pytest.mark.gpu
K = pr.K


def join(ctx, idx, metric, D, **shard):
    return gj.join(ctx, idx, metric, D, K, **shard)


def assert_shards(ctx, idx, metric, D, want, shards):
    gj.assert_shards(ctx, idx, metric, D, K, want, shards)


def build(ctx, key):
    h, off, bits = pr.collection(key)[:3]
    idx = ctx.index_build(ctx.sketches_from_host(h, off), bits)
    assert np.array_equal(idx.order, np.arange(len(off) - 1))
    return idx


# ---- 2. tiles that hold exactly one cell: the counting loop at its smallest sizes, the launch prefix -----------------------
@pytest.mark.parametrize("from_build", ["0", "1"])
@pytest.mark.parametrize("threads", ["256", "512", "1024"])
def test_tiles_of_one_cell(monkeypatch, threads, from_build):
    """Seventeen identical pairs of 1 .. 1,025 hashes, each alone in its tile (row 31 against column 0, the partial last block,
    a diagonal tile): a tile has exactly `common` records and one non-zero cell, so a record dropped or counted twice at the
    end of a wave's share (one record per workgroup, an odd count under the scalar row masks, a share that ends on a
    128-record step) is a wrong `common`.  Records from the lazy builder and from the build; the directory against the model."""
    h, off, bits, pairs = pr.cells_collection()
    t = pr.tiles(h, off)
    assert dict(zip(t["keys"], t["records"].tolist())) == {(i >> 5, j >> 5): c for i, j, c in pairs} and len(t["keys"]) == 17
    ctx = make_ctx(monkeypatch, {"RK_DIST_TILES": "1", "RK_INDEX_TILES": from_build})
    monkeypatch.setenv("RK_TILE_THREADS", threads)
    try:
        idx = build(ctx, ("cells",))
        assert idx.products == (6 if from_build == "1" else 1)
        for srow in ("false", "true"):
            monkeypatch.setenv("RK_TILE_SROW", "1" if srow == "true" else "0")
            for metric in (0, 1):
                for D in (0.05, 0.3):
                    want = pr.oracle_hits(("cells",), metric, D)
                    assert pairs_of(want) == {(i, j) for i, j, _ in pairs}
                    assert_hits_equal(join(ctx, idx, metric, D), want)
                    assert ctx.dist_kernel_name(idx, None, 1, metric, K, D) == "rk_tile_kernel<%su, %s>" % (threads, srow)
                    grid, rel = pr.launch_grid(t, metric, D)
                    assert rel > 1e-5
                    stats = idx.tile_stats(1, metric, K, D)
                    assert (stats[0], stats[1], stats[2]) == (17, grid, sum(pr.COMMONS)), stats
            assert_shards(ctx, idx, 0, 0.05, pr.oracle_hits(("cells",), 0, 0.05), ((3, 16), (2, 64), (5, 1)))
        del idx
    finally:
        ctx.close()


# ---- 3. tiles on the bound: the launch prefix, the `take` test, lb, the level table ------------------------------------------
@pytest.mark.parametrize("from_build", ["0", "1"])
def test_tiles_on_the_bound(monkeypatch, from_build):
    """Pairs alone in their tiles whose ratio records / lb is tight against min_jorc: for every D one with first_reportable
    hashes (reported) and one with one fewer (not); jaccard subsets (lb: the row's size), containment pairs of equal sizes, and
    a row three times its column (lb: the smaller block minimum); thresholds on either side of four levels of the directory's
    table, where the last level a launch covers holds a reported pair.  An empty and a one-hash sketch share blocks with
    designated pairs: min_ref_size is 1, block minima ignore the empty one."""
    h, off, bits, pairs = pr.bounds_collection()
    sizes = np.diff(off).astype(np.int64)
    assert sizes[sizes > 0].min() == pr.BOUND_MIN_REF_SIZE == 1 and sizes.min() == 0
    t = pr.tiles(h, off)
    at = {k: x for x, k in enumerate(t["keys"])}
    assert len(at) == len(pairs) and all(t["records"][at[(i >> 5, j >> 5)]] == spec[5] for i, j, spec in pairs)
    for D in pr.BOUND_D:
        assert pr.first_reportable(0, D, pr.BOUND_S, "subset") == pr.floor_common(0, D, pr.BOUND_S, 1) + 1
    for k in pr.LEVELS:
        tight, loose = pr.level_thresholds(k)
        assert (pr.launch_kk(0, tight), pr.launch_kk(0, loose)) == (k, k + 1)
        required = pairs_of(pr.oracle_hits(("bounds",), 0, tight))
        assert any(pr.tile_levels(t, 0)[at[(i >> 5, j >> 5)]] == k for i, j in required)    # the last level the launch covers
    ctx = make_ctx(monkeypatch, {"RK_DIST_TILES": "1", "RK_INDEX_TILES": from_build})
    try:
        idx = build(ctx, ("bounds",))
        assert idx.products == (6 if from_build == "1" else 1)
        for metric, D in pr.bound_thresholds():
            want = pr.oracle_hits(("bounds",), metric, D)
            got = pairs_of(want)
            for i, j, (kind, m, d, s0, rule, c) in pairs:
                if (m, d) == (metric, D):
                    assert ((i, j) in got) == (c == pr.first_reportable(m, d, s0, rule))
            grid, rel = pr.launch_grid(t, metric, D)
            assert rel > 1e-5       # no tile within float rounding of a level: the model's grid is exact
            for srow in ("0", "1"):
                monkeypatch.setenv("RK_TILE_SROW", srow)
                assert_hits_equal(join(ctx, idx, metric, D), want)
                assert ctx.dist_kernel_name(idx, None, 1, metric, K, D).endswith(", true>" if srow == "1" else ", false>")
            monkeypatch.delenv("RK_TILE_SROW")
            stats = idx.tile_stats(1, metric, K, D)
            assert (stats[0], stats[1], stats[2]) == (len(at), grid, int(t["records"].sum())), (metric, D, stats)
            monkeypatch.setenv("RK_TILE_ALL", "1")      # every tile gets a workgroup: the kernel's own test is the only prune
            assert idx.tile_stats(1, metric, K, D)[1] == len(at)
            assert_hits_equal(join(ctx, idx, metric, D), want)
            monkeypatch.delenv("RK_TILE_ALL")
        del idx
    finally:
        ctx.close()


# ---- 4. the window and the far-record bound of rk_near_kernel ---------------------------------------------------------------
def site_conditions(kind, metric, pair):
    """(h, off, D, the oracle's hits, units the model sends to the fallback); the collection's conditions, asserted again"""
    h, off, _ = pr.sites_collection(kind, metric)
    D, mrs = pr.SITE_D[metric], pr.site_min_ref_size(kind, metric)
    fc, fr = pr.site_counts(metric)
    assert fr == fc + 1 and np.diff(off).min() == mrs
    assert math.floor(pr.min_jorc(metric, D) * mrs) >= 16      # (RK_DIST_NEAR_MIN: or the plan never takes rk_near_kernel)
    want = pr.oracle_hits(("sites", kind, metric), metric, D)
    got = pairs_of(want)
    for s, (odd, size, rels) in enumerate(pr.site_specs(kind, metric)):   # first_reportable hashes: reported; one fewer: not
        first = pr.SITE_STRIDE * s + 10
        for col, cnt, _ in rels:
            assert ((first + odd, first + col) in got) == (cnt >= fr)
    return h, off, D, want, pr.falls_back(h, off, metric, D, mrs, pair)


@pytest.mark.parametrize("pair", ["default", "2"])
@pytest.mark.parametrize("uw", ["1", "2", "4"])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", ["quiet", "loud"])
def test_near_window_on_its_bounds(monkeypatch, kind, metric, uw, pair):
    """Sites 80 ids apart: a row of 1,000 hashes (3,000 for the containment site whose row is three times its columns), relatives
    with first_reportable hashes on the window's first and last column -- for a unit's first row and for its partner --, far
    genomes from the first column behind the window on.  Quiet: every far genome holds floor_common - 1 hashes of its row,
    nothing falls back.  Loud: floor_common (falls back, not reported), first_reportable (reported; 33 columns behind the first
    row, 32 behind the partner), first_reportable - 1 and 1 over two genomes, and hashes held by the first row, its partner
    and a far genome (the shared slices).  One more site on the last two rows of the odd-sized collection."""
    h, off, D, want, fb = site_conditions(kind, metric, pair == "default")
    assert (fb == []) == (kind == "quiet")
    env = {"RK_DIST_TILES": "0", "RK_DIST_NEAR_UW": uw}
    if pair != "default":
        env["RK_DIST_PAIR"] = pair
    ctx = make_ctx(monkeypatch, env)
    try:
        idx = build(ctx, ("sites", kind, metric))
        name = "rk_near_kernel<%s, %s>" % ("true" if pair == "default" else "false", uw)
        assert ctx.dist_kernel_name(idx, None, 1, metric, K, D) == name
        for _ in range(3):      # (the second resets the fallback list, the third may skip an empty fallback launch)
            assert_hits_equal(join(ctx, idx, metric, D), want)
        assert_shards(ctx, idx, metric, D, want, ((3, 16),))
        assert ctx.dist_kernel_name(idx, None, 1, metric, K, D) == name
        del idx
    finally:
        ctx.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", ["quiet", "edge", "loud"])
def test_a_unit_falls_back_exactly_when_the_model_says_so(monkeypatch, kind, metric):
    """Default switches: once a completed join has found rows in the fallback list, later joins take the tile kernel -- so the
    name tells whether any unit fell back.  Quiet: none (the name stays).  Edge: the quiet collection and ONE site whose far
    genome holds exactly floor_common hashes of its row (the name moves).  Loud: several."""
    h, off, D, want, fb = site_conditions(kind, metric, True)
    assert (fb == []) == (kind == "quiet") and (kind != "edge" or len(fb) == 1)
    ctx = make_ctx(monkeypatch, {})
    try:
        idx = build(ctx, ("sites", kind, metric))
        seen = []
        for _ in range(3):
            seen.append(ctx.dist_kernel_name(idx, None, 1, metric, K, D).split("<")[0])
            assert_hits_equal(join(ctx, idx, metric, D), want)
        seen.append(ctx.dist_kernel_name(idx, None, 1, metric, K, D).split("<")[0])
        assert seen[0] == "rk_near_kernel", seen
        assert seen[-1] == ("rk_tile_kernel" if fb else "rk_near_kernel"), seen
        assert_hits_equal(join(ctx, idx, metric, D), want)
        del idx
    finally:
        ctx.close()


# ---- 5. the candidate list of rk_dist_kernel --------------------------------------------------------------------------------
BANDS = {"RK_DIST_BAND_MIN_ROWS": "64", "RK_DIST_LDS_KB": "12"}    # an LDS row of 512 columns: the first rows in tiles, the last in one
SITE_JOINS = {m: [(m, pr.SITE_D[m])] for m in (0, 1)}
CELL_JOINS = [(0, 0.05), (0, 0.3), (1, 0.05)]
BOUND_JOINS = [(m, D) for m in (0, 1) for D in pr.BOUND_D]
DIST_CASES = {
    # collection, switches, joins, what the name must hold
    "cells": (("cells",), {}, CELL_JOINS, "rk_dist_kernel<true, 2, "),
    "cells_in_bands": (("cells",), BANDS, CELL_JOINS, " bands]"),
    "bounds": (("bounds",), {}, BOUND_JOINS, "rk_dist_kernel<true, 2, "),
    "bounds_in_bands": (("bounds",), BANDS, BOUND_JOINS, " bands]"),
    "bounds_single_rows": (("bounds",), {"RK_DIST_PAIR": "2"}, BOUND_JOINS, "rk_dist_kernel<true, 1, "),
    "sites_jaccard": (("sites", "loud", 0), {}, SITE_JOINS[0], "rk_dist_kernel<true, 2, "),
    "sites_containment": (("sites", "loud", 1), {}, SITE_JOINS[1], "rk_dist_kernel<true, 2, "),
    "sites_containment_single_rows": (("sites", "loud", 1), {"RK_DIST_PAIR": "2"}, SITE_JOINS[1], "rk_dist_kernel<true, 1, "),
    # one sketch of 66,000 hashes: 32-bit counters
    "sites_jaccard_u32": (("sites", "loud", 0, True), {}, SITE_JOINS[0], "rk_dist_kernel<false, "),
    "sites_containment_u32": (("sites", "loud", 1, True), {}, SITE_JOINS[1], "rk_dist_kernel<false, "),
}


@pytest.mark.parametrize("case", list(DIST_CASES))
def test_candidate_list_on_the_row_bound(monkeypatch, case):
    """The collections above through the kernel with full counter rows (RK_DIST_NEAR=0 RK_DIST_TILES=0): cells with
    first_reportable hashes enter the candidate list, for 16- and 32-bit counters, row pairs and single rows, bands -- also
    where the row is three times its column and the bound comes from the smallest sketch, not from the row."""
    key, env, joins, name = DIST_CASES[case]
    if key[0] == "sites":
        site_conditions(key[1], key[2], True)
        assert (np.diff(pr.collection(key)[1]).max() >= 65536) == (len(key) == 4)
    ctx = make_ctx(monkeypatch, dict(env, RK_DIST_NEAR="0", RK_DIST_TILES="0"))
    try:
        idx = build(ctx, key)
        for metric, D in joins:
            want = pr.oracle_hits(key, metric, D)
            assert len(want) > 0
            got = ctx.dist_kernel_name(idx, None, 1, metric, K, D)
            assert got.startswith("rk_dist_kernel<") and name in got, got
            assert_hits_equal(join(ctx, idx, metric, D), want)
            assert_hits_equal(join(ctx, idx, metric, D), want)
        assert_shards(ctx, idx, joins[0][0], joins[0][1], pr.oracle_hits(key, *joins[0]), ((3, 16),))
        del idx
    finally:
        ctx.close()


# ---- every collection once with the index's own numbering: results only -----------------------------------------------------
@pytest.mark.parametrize("key,joins", [(("cells",), CELL_JOINS), (("bounds",), BOUND_JOINS), (("sites", "quiet", 0), SITE_JOINS[0]),
                                       (("sites", "loud", 0), SITE_JOINS[0]), (("sites", "loud", 1), SITE_JOINS[1])],
                         ids=["cells", "bounds", "sites_quiet", "sites_loud_jaccard", "sites_loud_containment"])
def test_collections_with_renumbering_on(monkeypatch, key, joins):
    ctx = make_ctx(monkeypatch, {}, relabel=True)
    try:
        h, off, bits = pr.collection(key)[:3]
        idx = ctx.index_build(ctx.sketches_from_host(h, off), bits)
        for metric, D in joins:
            for _ in range(2):
                assert_hits_equal(join(ctx, idx, metric, D), pr.oracle_hits(key, metric, D))
        del idx
    finally:
        ctx.close()
