"""The ladder of the self join (rk_dist.hip plan_self), one small case per rung: which kernel rk_dist_kernel_name reports before
the first join and after it -- literals recorded on the commit before plan_self existed -- and the oracle's hits from two joins
in a row.  Small collections (240 to 3,000 synthetic genomes, sketches of 40 to 200 hashes), developer switches bring the rungs
down to them; the switches are read when a context is created."""
import functools

import numpy as np
import pytest

from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
K = 20


@functools.lru_cache(maxsize=None)
def collection(kind):
    if kind == "multiset":   # some hashes two or three times in a genome: counts are products of multiplicities
        rng = np.random.default_rng(5)
        parts = []
        for _ in range(240):
            base = np.unique(rng.integers(0, 1 << 16, size=120, dtype=np.uint64).astype(np.uint32))
            parts.append(np.sort(np.concatenate([base, rng.choice(base, size=int(rng.integers(1, 12)), replace=True)])).astype(np.uint32))
        h, off, bits = np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64), 16
    else:
        n, m, bits, strains = {"clades10": (1500, 200, 26, 10), "clades70": (1400, 120, 26, 70), "small": (300, 150, 24, 10),
                               "short": (3000, 40, 24, 10)}[kind]
        names, h, off = synth.clade_sketches(n, m, bits, strains_per_clade=strains, seed=1000 + n)
        names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(n, "shuffled", seed=strains))
    for a in (h, off):
        a.setflags(write=False)
    return h, off, bits


@functools.lru_cache(maxsize=None)
def oracle_hits(kind, metric, D):
    h, off, bits = collection(kind)
    postings, counts = ok.index_build32(h, off, bits)
    want, _ = ok.index_dist32(counts, bits, postings, np.diff(off).astype(np.uint32), h, off, 1, metric, K, D, threads=4)
    want.setflags(write=False)
    return want


# case: collection, switches, (metric, D), row shards (row_step, row_block), thresholds joined first (they leave their lazy
# products in the index), (name before the first join, name after it)
CASES = {
    # the build emits tile records (as from 4,000 genomes on): the tile kernel from the first join
    "tile_records_from_the_build": ("clades10", {"RK_DIST_TILES_MIN_GENOMES": "1000"}, (0, 0.05), (1, 0), (), ("rk_tile_kernel<1024u, false>", "rk_tile_kernel<1024u, false>")),
    "tiles_forced": ("clades10", {"RK_DIST_TILES": "1"}, (0, 0.05), (1, 0), (), ("rk_tile_kernel", "rk_tile_kernel<1024u, false>")),
    "tiles_off": ("clades70", {"RK_DIST_TILES": "0"}, (0, 0.05), (1, 0), (), ("rk_near_kernel<true, 2>", "rk_near_kernel<true, 2>")),
    "near_off": ("clades10", {"RK_DIST_NEAR": "0"}, (0, 0.05), (1, 0), (), ("rk_dist_kernel<true, 2, 512>", "rk_dist_kernel<true, 2, 512>")),
    # floor(min_jorc * smallest sketch) = 0 < RK_DIST_NEAR_MIN: tile records on first use
    "loose_threshold": ("clades10", {}, (0, 0.3), (1, 0), (), ("rk_tile_kernel", "rk_tile_kernel<1024u, false>")),
    "default_small_clades": ("clades10", {}, (0, 0.05), (1, 0), (), ("rk_near_kernel<true, 2>", "rk_near_kernel<true, 2>")),
    # clades of 70: most slice records reach beyond the 32-column window (`spread`)
    "clades_wider_than_the_window": ("clades70", {}, (0, 0.05), (1, 0), (), ("rk_tile_kernel", "rk_tile_kernel<1024u, false>")),
    # tile AND slice records (the loose join made the tile records): a quarter of the rows prefers the near-window kernel ...
    "small_shard": ("clades10", {}, (0, 0.05), (4, 32), (0.3,), ("rk_near_kernel<true, 2>", "rk_near_kernel<true, 2>")),
    # ... but not in the join that makes the tile records (a fresh index, the loose threshold asks for them): that one runs on them
    "small_shard_first_join": ("clades10", {}, (0, 0.3), (4, 32), (), ("rk_tile_kernel", "rk_dist_kernel<true, 2, 512>")),
    "whole_of_the_same_index": ("clades10", {}, (0, 0.05), (1, 0), (0.3,), ("rk_tile_kernel<1024u, false>", "rk_tile_kernel<1024u, false>")),
    # ... unless the index has no slice records
    "small_shard_without_slice_records": ("clades10", {"RK_DIST_TILES_MIN_GENOMES": "1000"}, (0, 0.05), (4, 32), (), ("rk_tile_kernel<1024u, false>", "rk_tile_kernel<1024u, false>")),
    "no_slice_records_possible": ("clades10", {"RK_INDEX_NO_SELF": "1"}, (1, 0.08), (1, 0), (), ("rk_tile_kernel<1024u, false>", "rk_tile_kernel<1024u, false>")),
    "repeated_hashes": ("multiset", {}, (0, 0.2), (1, 0), (), ("rk_dist_kernel<false, 1, 256>", "rk_dist_kernel<false, 1, 256>")),
    "dense_report": ("small", {}, (0, 1.5), (1, 0), (), ("rk_dist_kernel<true, 2, 512>", "rk_dist_kernel<true, 2, 512>")),
    "bands": ("short", {"RK_DIST_NEAR": "0", "RK_DIST_BAND_MIN_ROWS": "64", "RK_DIST_LDS_KB": "16"}, (0, 0.05), (1, 0), (), ("rk_dist_kernel<true, 0, 256> [2 bands]", "rk_dist_kernel<true, 0, 256> [2 bands]")),
    # tile records from the build, the tile kernel switched off: the first join makes the slice records and runs on the
    # near-window kernel -- and that is the name before it too (until plan_self the name before was rk_dist_kernel<true, 1, 256>:
    # the name's copy of the ladder did not know that the launch makes the records)
    "slice_records_on_first_use": ("clades10", {"RK_DIST_TILES_MIN_GENOMES": "1000", "RK_DIST_TILES": "0"}, (0, 0.05), (1, 0), (), ("rk_near_kernel<true, 2>", "rk_near_kernel<true, 2>")),
}


def join_case(case, setenv):
    """([name before the first join, after it, after the second], [hits of the first join, of the second])"""
    kind, env, (metric, D), (step, block), first, _ = CASES[case]
    for k, v in env.items():
        setenv(k, v)
    ctx = capi.Context(0)
    try:
        h, off, bits = collection(kind)
        idx = ctx.index_build(ctx.sketches_from_host(h, off), bits)
        for d in first:
            ctx.dist_rows(idx, None, 1, metric, K, d)
        names, hits = [], []
        for _ in range(2):
            names.append(ctx.dist_kernel_name(idx, None, 1, metric, K, D, row_first=step - 1, row_step=step, row_block=block))
            merged = np.concatenate([ctx.dist_rows(idx, None, 1, metric, K, D, row_first=r, row_step=step, row_block=block)[0] for r in range(step)])
            hits.append(merged[np.lexsort((merged["col"], merged["row"]))])
        names.append(ctx.dist_kernel_name(idx, None, 1, metric, K, D, row_first=step - 1, row_step=step, row_block=block))
        del idx
    finally:
        ctx.close()
    return names, hits


@pytest.mark.parametrize("case", list(CASES))
def test_self_join_plan(monkeypatch, case):
    kind, _, (metric, D), _, _, (before, after) = CASES[case]
    want = oracle_hits(kind, metric, D)
    assert len(want) > 0
    names, hits = join_case(case, monkeypatch.setenv)
    assert names == [before, after, after]
    for mine in hits:
        assert len(mine) == len(want)
        for f in ("row", "col", "common", "size0", "size1", "jorc", "dist"):
            assert np.array_equal(mine[f], want[f]), f


def test_first_join_of_a_small_shard_runs_the_kernel_it_was_named(monkeypatch, capfd):
    # A fresh index with slice records, a threshold that asks for tile records, a quarter of the rows: the name says rk_tile_kernel, and
    # the join that builds the records runs on them (as before plan_self) -- only later joins of the shard take counter rows.
    # RK_DIST_DEBUG prints one line per band of a counter-row plan that is launched or named: that tells which kernel ran.
    monkeypatch.setenv("RK_DIST_DEBUG", "1")
    ctx = capi.Context(0)
    try:
        h, off, bits = collection("clades10")
        idx = ctx.index_build(ctx.sketches_from_host(h, off), bits)
        shard = dict(row_step=4, row_block=32)
        assert ctx.dist_kernel_name(idx, None, 1, 0, K, 0.3, row_first=3, **shard) == "rk_tile_kernel"
        capfd.readouterr()
        parts = [ctx.dist_rows(idx, None, 1, 0, K, 0.3, row_first=3, **shard)[0]]
        assert capfd.readouterr().err.count("band:") == 0 and idx.products & 2
        assert ctx.dist_kernel_name(idx, None, 1, 0, K, 0.3, row_first=3, **shard) == "rk_dist_kernel<true, 2, 512>"
        capfd.readouterr()
        parts += [ctx.dist_rows(idx, None, 1, 0, K, 0.3, row_first=r, **shard)[0] for r in range(3)]
        assert capfd.readouterr().err.count("band:") == 3
        merged = np.concatenate(parts)
        merged, want = merged[np.lexsort((merged["col"], merged["row"]))], oracle_hits("clades10", 0, 0.3)
        for f in ("row", "col", "common", "size0", "size1", "jorc", "dist"):
            assert np.array_equal(merged[f], want[f]), f
        del idx
    finally:
        ctx.close()
