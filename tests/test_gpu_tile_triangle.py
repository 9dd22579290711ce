"""rk_tile_kernel (rabbitkssd_amd/csrc/rk_dist_tile.inc) where a DIAGONAL tile is evaluated as a triangle -- its 496
cells with col > row, numbered by rk_tile_cells.h, in ceil(496 / threads) rounds -- and where the waves of a workgroup take their
shares of a tile's records (even ones in whole groups of 16 at eight and sixteen waves, whole steps of 128 at four); against the oracle (ok.index_build32 / ok.index_dist32): integers equal, jorc
and dist bit for bit.

    seam                                                              leg
    all 496 cells of tile (0, 0) are hits, (0, 1), (0, 31), (30, 31)   test_every_cell_of_a_diagonal_tile
    more hits than the caller's buffer holds                          test_every_cell_of_a_diagonal_tile (rk_dist_rows_dev)
    a partial last diagonal tile; an off-diagonal tile beside two     test_partial_and_neighbouring_tiles
      diagonal ones
    orig relabel, row / col flip                                      test_shuffled_order
    a shard edge inside a tile, shards whose union is the whole       test_row_shards
    two joins on one index at different -D                            test_joins_back_to_back
    a wave's share at group, step and wave edges (4, 8, 16 waves)     test_tiles_of_n_records

Every collection gives every genome a size of its own and every cell a count that depends on both members, so a cell evaluated
under another's number shows in common, size0 or size1.  Every leg runs RK_TILE_THREADS in {256, 512, 1024} (parametrised),
RK_TILE_SROW in {0, 1} and both metrics, and asserts the variant it ran (rk_dist_kernel_name)."""
import functools

import numpy as np
import pytest

from oracle import oracle as ok

import _gpu_join as gj
import _prune_ref as pr
import _rows_ref as rr
from _gpu_join import assert_hits_equal, make_ctx

pytestmark = pytest.mark.gpu
K = pr.K
BITS = pr.BITS
D = 0.05
TIGHT = {0: 0.001, 1: 0.00037}   # thresholds that report part of near_collection(64), per metric
CORE = 300                  # hashes of the shared core: genome g holds the first CORE - g of them
THREADS = ["256", "512", "1024"]
RECORDS = (1, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 4735, 4736, 4737)
TAGS = 16                    # kMinK of rk_index.hip: the smallest hashes of a sketch decide its cluster


def freeze(h, off):
    for a in (h, off):
        a.setflags(write=False)
    return h, off


@functools.lru_cache(maxsize=None)
def near_collection(n):
    """n near-identical sketches: genome g holds the first CORE - g hashes of one core and two of its own -- sizes
    CORE + 2 - g, common(i, j) = CORE - max(i, j): every pair is reportable under D for both metrics"""
    assert n <= 64
    pool = rr.Ascending()
    core = pool.take(CORE)
    return freeze(*pr.csr([np.concatenate([core[:CORE - g], pool.take(2)]) for g in range(n)]))


@functools.lru_cache(maxsize=None)
def shuffled_collection():
    """the 64 sketches of near_collection with 16 smallest hashes on top, one set for the even genomes and one for the odd ones
    -- the index's renumbering keeps the genomes that share their smallest hashes together, so the internal order is evens,
    then odds, and a pair (odd i, even j > i) is counted as (row j, col i) and reported flipped --, listed in a shuffled order"""
    n = 64
    pool = rr.Ascending()
    core = pool.take(CORE)
    tags = (np.arange(1, 1 + TAGS, dtype=np.uint32), np.arange(101, 101 + TAGS, dtype=np.uint32))
    assert tags[1].max() < core.min()
    parts = [np.concatenate([tags[g % 2], core[:CORE - g], pool.take(2)]) for g in range(n)]
    order = np.random.default_rng(20261021).permutation(n)
    return freeze(*pr.csr([parts[g] for g in order]))


@functools.lru_cache(maxsize=None)
def records_collection():
    """26 blocks of 32 sketches of one private hash; for every n of RECORDS (the p-th) two identical pairs of n hashes, each pair
    alone in its tile: one inside block p -- the DIAGONAL tile (p, p) holds n records -- and one between block p and block
    13 + p -- the tile (p, 13 + p) holds n records.  (h, off, [(i, j, n)])"""
    nb = 2 * len(RECORDS)
    pool, parts, pairs = pr.Hashes(), [None] * (32 * nb), []
    for p, c in enumerate(RECORDS):
        for i, j in ((32 * p + 3, 32 * p + 28), (32 * p + 7, 32 * (len(RECORDS) + p) + 9)):
            parts[i] = pool.take(c)
            parts[j] = parts[i].copy()
            pairs.append((i, j, c))
    for g in range(len(parts)):
        if parts[g] is None:
            parts[g] = pool.take(1)
    h, off = freeze(*pr.csr(parts))
    return h, off, tuple(pairs)


COLLECTIONS = {"near": near_collection, "shuffled": shuffled_collection, "records": records_collection}


@functools.lru_cache(maxsize=None)
def oracle_index(key):
    h, off = COLLECTIONS[key[0]](*key[1:])[:2]
    return ok.index_build32(h, off, BITS)


@functools.lru_cache(maxsize=None)
def oracle_hits(key, metric, max_dist):
    h, off = COLLECTIONS[key[0]](*key[1:])[:2]
    postings, counts = oracle_index(key)
    want, _ = ok.index_dist32(counts, BITS, postings, np.diff(off).astype(np.uint32), h, off, 1, metric, K, max_dist, threads=8)
    want.setflags(write=False)
    return want


def tile_ctx(monkeypatch, threads, relabel=False):
    ctx = make_ctx(monkeypatch, {"RK_DIST_TILES": "1"}, relabel=relabel)
    monkeypatch.setenv("RK_TILE_THREADS", threads)     # (read at every launch, as RK_TILE_SROW)
    return ctx


def variants(monkeypatch):
    """every (srow, metric); RK_TILE_SROW is set for the leg that follows"""
    for srow in ("false", "true"):
        monkeypatch.setenv("RK_TILE_SROW", "1" if srow == "true" else "0")
        for metric in (0, 1):
            yield srow, metric


def join_and_name(ctx, idx, metric, max_dist, threads, srow, **shard):
    got = gj.join(ctx, idx, metric, max_dist, K, **shard)
    assert ctx.dist_kernel_name(idx, None, 1, metric, K, max_dist) == "rk_tile_kernel<%su, %s>" % (threads, srow)
    return got


def build(ctx, key, identity=True):
    h, off = COLLECTIONS[key[0]](*key[1:])[:2]
    idx = ctx.index_build(ctx.sketches_from_host(h, off), BITS)
    assert np.array_equal(idx.order, np.arange(len(off) - 1)) == identity
    return idx


def all_pairs(n):
    return {(i, j) for i in range(n) for j in range(i + 1, n)}


# ---- every cell of a diagonal tile ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
def test_every_cell_of_a_diagonal_tile(monkeypatch, threads):
    """32 near-identical sketches: one tile, (0, 0), whose 496 cells above the diagonal are all hits -- the first and the last
    number of the triangle, the corners (0, 1), (0, 31) and (30, 31), and at 256 threads both rounds.  Then through
    rk_dist_rows_dev with room for 100 and for 495 records: the counter reports all 496, the records written are distinct
    members of the result, the guard behind the buffer is untouched."""
    key = ("near", 32)
    h, off = near_collection(32)
    t = pr.tiles(h, off)
    assert t["keys"] == [(0, 0)] and t["records"].tolist() == [CORE - 1]    # (the last core hash is genome 0's alone)
    ctx = tile_ctx(monkeypatch, threads)
    try:
        idx = build(ctx, key)
        for srow, metric in variants(monkeypatch):
            want = oracle_hits(key, metric, D)
            assert gj.pairs_of(want) == all_pairs(32) and len(want) == 496
            cells = rr.hit_cells(want)
            assert (cells[(0, 1)], cells[(0, 31)], cells[(30, 31)]) == (CORE - 1, CORE - 31, CORE - 31)
            assert_hits_equal(join_and_name(ctx, idx, metric, D, threads, srow), want)
            for cap in (100, 495):
                n, got = gj.dev_records(ctx, idx, None, 1, metric, D, K, cap)      # (asserts the guard)
                gj.assert_capped_records(n, got, want, cap, 32)
        del idx
    finally:
        ctx.close()


# ---- a partial last diagonal tile, an off-diagonal tile beside two diagonal ones -----------------------------------------------
@pytest.mark.parametrize("n", [40, 64])
@pytest.mark.parametrize("threads", THREADS)
def test_partial_and_neighbouring_tiles(monkeypatch, threads, n):
    """40 genomes: the diagonal tile (1, 1) holds 8 genomes -- 28 of its 496 numbers are cells of the collection (gcol < n_ref
    rejects the others); 64: two whole diagonal tiles and the off-diagonal tile (0, 1) between them, whose 1,024 cells are
    all hits and keep their own numbering.  Every pair is reported."""
    key = ("near", n)
    h, off = near_collection(n)
    assert pr.tiles(h, off)["keys"] == [(0, 0), (0, 1), (1, 1)]
    ctx = tile_ctx(monkeypatch, threads)
    try:
        idx = build(ctx, key)
        for srow, metric in variants(monkeypatch):
            want = oracle_hits(key, metric, D)
            assert gj.pairs_of(want) == all_pairs(n)
            assert_hits_equal(join_and_name(ctx, idx, metric, D, threads, srow), want)
        del idx
    finally:
        ctx.close()


# ---- the caller's order differs from the internal one --------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
def test_shuffled_order(monkeypatch, threads):
    """The renumbered index of shuffled_collection: hits carry the caller's ids (orig), and a pair whose members stand the other
    way round in the internal order is reported flipped -- asserted from rk_index_order before the hits are compared."""
    key = ("shuffled",)
    ctx = tile_ctx(monkeypatch, threads, relabel=True)
    try:
        idx = build(ctx, key, identity=False)
        inv = np.empty(64, dtype=np.int64)
        inv[idx.order] = np.arange(64)
        for srow, metric in variants(monkeypatch):
            want = oracle_hits(key, metric, D)
            assert gj.pairs_of(want) == all_pairs(64)
            flipped = inv[want["row"]] > inv[want["col"]]
            assert flipped.sum() >= 64 and (~flipped).sum() >= 64
            assert_hits_equal(join_and_name(ctx, idx, metric, D, threads, srow), want)
        del idx
    finally:
        ctx.close()


# ---- row shards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
def test_row_shards(monkeypatch, threads):
    """64 genomes in row shards of blocks of 16 rows (a shard edge inside every tile: a diagonal tile's triangle is cut by
    rows) and of 32 rows (whole tiles), dealt to 2 and 3 shards: every hit comes from the shard of its row, the union is the
    whole."""
    key = ("near", 64)
    ctx = tile_ctx(monkeypatch, threads)
    try:
        idx = build(ctx, key)
        for srow, metric in variants(monkeypatch):
            want = oracle_hits(key, metric, D)
            assert_hits_equal(join_and_name(ctx, idx, metric, D, threads, srow), want)
            gj.assert_shards(ctx, idx, metric, D, K, want, ((2, 16), (3, 16), (2, 32), (3, 32)))
        del idx
    finally:
        ctx.close()


# ---- two joins on one index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
def test_joins_back_to_back(monkeypatch, threads):
    """The same index joined under D, under a threshold that reports part of every tile, and under D again: a join leaves
    nothing behind that the next one counts."""
    key = ("near", 64)
    ctx = tile_ctx(monkeypatch, threads)
    try:
        idx = build(ctx, key)
        for srow, metric in variants(monkeypatch):
            tight = TIGHT[metric]
            loose, few = oracle_hits(key, metric, D), oracle_hits(key, metric, tight)
            assert 64 < len(few) < len(loose) // 2
            for max_dist, want in ((D, loose), (tight, few), (D, loose), (tight, few)):
                assert_hits_equal(join_and_name(ctx, idx, metric, max_dist, threads, srow), want)
        del idx
    finally:
        ctx.close()


# ---- even shares -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
def test_tiles_of_n_records(monkeypatch, threads):
    """Two identical sketches of n hashes alone in a tile: the tile holds n records and one non-zero cell, whose `common` is n
    only if every wave counted its share and no record twice.  n on either side of a group of 16 records, of a step of 128, of
    eight waves' steps (1,024) and of shares that end on a group (4,736 = 8 x 592 = 16 x 296 = 4 x 1,184) -- in a diagonal and
    in an off-diagonal tile."""
    key = ("records",)
    h, off, pairs = records_collection()
    t = pr.tiles(h, off)
    assert dict(zip(t["keys"], t["records"].tolist())) == {(i >> 5, j >> 5): c for i, j, c in pairs} and len(pairs) == 2 * len(RECORDS)
    assert sum(i >> 5 == j >> 5 for i, j, _ in pairs) == len(RECORDS)
    ctx = tile_ctx(monkeypatch, threads)
    try:
        idx = build(ctx, key)
        for srow, metric in variants(monkeypatch):
            want = oracle_hits(key, metric, D)
            assert rr.hit_cells(want) == {(i, j): c for i, j, c in pairs}
            got = join_and_name(ctx, idx, metric, D, threads, srow)
            assert rr.hit_cells(got) == {(i, j): c for i, j, c in pairs}
            assert_hits_equal(got, want)
        del idx
    finally:
        ctx.close()
