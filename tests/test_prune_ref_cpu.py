"""The model and the generators of tests/_prune_ref.py, checked on the CPU before a GPU is involved: `tiles` against a brute
force over all pairs, the generators' sketches (ascending sets with the intended intersections), and every condition the GPU
tests of tests/test_gpu_prune_edges.py rest on, for the shipped parameters (they assert them again)."""
import math

import numpy as np
import pytest

from oracle import oracle as ok

import _prune_ref as pr


def sketches(h, off):
    return [h[int(off[g]):int(off[g + 1])] for g in range(len(off) - 1)]


def assert_ascending_sets(h, off):
    for s in sketches(h, off):
        assert np.all(s[1:] > s[:-1])


def common(parts, i, j):
    return len(np.intersect1d(parts[i], parts[j], assume_unique=True))


def pairs_of(hits):
    return set(zip(hits["row"].tolist(), hits["col"].tolist()))


def test_hashes_never_repeat():
    pool = pr.Hashes(12)
    a = np.concatenate([pool.take(1000), pool.take(3000), pool.take(95)])
    assert len(np.unique(a)) == 4095 and a.max() < 1 << 12
    with pytest.raises(AssertionError):
        pool.take(1)


def test_min_jorc_and_floor_common_are_the_expressions_of_the_kernels():
    for metric, D in ((0, 0.05), (1, 0.05), (0, 0.3), (1, 0.02)):
        t = math.exp(-20 * D)
        assert pr.min_jorc(metric, D) == (t if metric else t / (2.0 - t)) * (1.0 - 1e-6)
    assert pr.floor_common(0, 0.05, 1000, 7) == math.floor(pr.min_jorc(0, 0.05) * 1000)      # jaccard: the row's size alone
    assert pr.floor_common(1, 0.05, 3000, 1000) == math.floor(pr.min_jorc(1, 0.05) * 1000)   # containment: min(row, smallest)
    assert pr.floor_common(1, 0.05, 500, 1000) == math.floor(pr.min_jorc(1, 0.05) * 500)
    assert pr.floor_common(0, 0.3, 10, 10) == 1 and pr.floor_common(1, 0.3, 0, 1) == 1        # never below one


def test_first_reportable_is_the_oracles_first():
    for metric, D, s0, rule in ((0, 0.05, 200, "subset"), (1, 0.05, 600, 200), (0, 0.1, 1000, "subset"), (1, 0.1, 1000, 1000)):
        c = pr.first_reportable(metric, D, s0, rule)
        size1 = (lambda x: x) if rule == "subset" else (lambda x: rule)
        assert ok.distance(c, s0, size1(c), metric, pr.K)[1] < D
        assert not ok.distance(c - 1, s0, size1(c - 1), metric, pr.K)[1] < D
    # the relation the issue measured, for jaccard subsets: one above the row bound
    got = [pr.first_reportable(0, D, s, "subset") for D in (0.02, 0.05, 0.1) for s in (200, 1000)]
    assert got == [101, 505, 46, 226, 15, 73]
    assert got == [pr.floor_common(0, D, s, 1) + 1 for D in (0.02, 0.05, 0.1) for s in (200, 1000)]


def test_tiles_against_a_brute_force_over_all_pairs():
    rng = np.random.default_rng(11)
    parts = [np.unique(rng.integers(0, 900, size=int(rng.integers(0, 60)))).astype(np.uint32) for _ in range(150)]
    parts[40] = np.zeros(0, dtype=np.uint32)
    parts[64:96] = [np.zeros(0, dtype=np.uint32)] * 32      # a block of empty sketches
    h, off = pr.csr(parts)
    t = pr.tiles(h, off)
    brute = pr.brute_force_tiles(h, off)
    assert dict(zip(t["keys"], t["records"].tolist())) == brute and len(brute) == 10      # (four blocks with sketches)
    sizes = np.diff(off).astype(np.int64)
    for b in range(5):
        s = sizes[b * 32:(b + 1) * 32]
        assert t["blk_min"][b] == (s[s > 0].min() if np.any(s > 0) else 0xFFFFFFFF)
    assert t["blk_min"][2] == 0xFFFFFFFF and not any(2 in k for k in t["keys"])
    for at, (b, w) in enumerate(t["keys"]):
        assert t["lb"][0][at] == max(t["blk_min"][b], t["blk_min"][w]) and t["lb"][1][at] == min(t["blk_min"][b], t["blk_min"][w])
    # far records against the sets themselves
    sets = [set(p.tolist()) for p in parts]
    for row in (0, 1, 33, 100, 101):
        for pair in (True, False):
            first = row & ~1 if pair else row
            want = sum(1 for x in sets[row] if any(x in sets[g] for g in range(first + 33, 150)))
            assert pr.far_records(h, off, row, pair) == want


def test_launch_grid_counts_the_tiles_at_or_above_the_level_of_the_threshold():
    t = dict(records=np.array([100, 50, 25, 1]), lb=(np.array([100, 100, 100, 100]), np.array([100, 100, 100, 100])))
    assert pr.tile_levels(t, 0).tolist() == [0, 8, 16, 54]         # 2^(-k/8) <= ratio, less the margin
    theta = pr.thresholds()
    assert theta.dtype == np.float32 and theta[8] == np.float32(0.5) * (np.float32(1) - np.float32(1e-4))
    D = -math.log(2 * 0.5 / 1.5) / 20                               # jaccard 0.5: min_jorc a millionth below -> level 9
    assert pr.launch_kk(0, D) == 9 and pr.launch_grid(t, 0, D)[0] == 2
    assert pr.launch_kk(0, D * 0.98) == 8 and pr.launch_grid(t, 0, D * 0.98)[0] == 2      # level 8 is inclusive
    assert pr.launch_kk(0, D * 0.8) == 7 and pr.launch_grid(t, 0, D * 0.8)[0] == 1
    assert pr.launch_grid(t, 0, 2.0)[0] == 4                        # kk >= 256: every tile
    assert abs(pr.launch_grid(t, 0, D)[1] - 1e-4) < 1e-6            # the tiles that sit on 2^(-k/8) are the margin away


def test_cells_collection():
    h, off, bits, pairs = pr.cells_collection()
    assert len(off) - 1 == 761 and len(h) < 1_200_000 and bits <= 26
    assert_ascending_sets(h, off)
    assert len(np.unique(h)) == len(h) - sum(pr.COMMONS)            # nothing shared but the pairs
    parts = sketches(h, off)
    assert [c for _, _, c in pairs] == list(pr.COMMONS)
    for i, j, c in pairs:
        assert np.array_equal(parts[i], parts[j]) and len(parts[i]) == c
    t = pr.tiles(h, off)
    assert t["keys"] == sorted((i >> 5, j >> 5) for i, j, _ in pairs) and len(set(t["keys"])) == 17      # no two pairs in a tile
    assert dict(zip(t["keys"], t["records"].tolist())) == {(i >> 5, j >> 5): c for i, j, c in pairs}
    assert all(i >> 5 < 12 <= j >> 5 for i, j, _ in pairs[:16]) and pairs[16][0] >> 5 == pairs[16][1] >> 5
    assert sum(1 for i, j, _ in pairs if i % 32 == 31 and j % 32 == 0) >= 3
    assert sum(1 for _, j, _ in pairs if j >> 5 == 23) >= 1 and 761 % 32 != 0
    for metric, D in ((0, 0.05), (0, 0.3), (1, 0.05), (1, 0.3)):
        grid, rel = pr.launch_grid(t, metric, D)
        assert grid == 17 and rel > 1e-5
        want = pr.oracle_hits(("cells",), metric, D)
        assert pairs_of(want) == {(i, j) for i, j, _ in pairs} and sorted(want["common"].tolist()) == sorted(pr.COMMONS)


def test_bounds_collection():
    h, off, bits, pairs = pr.bounds_collection()
    n = len(off) - 1
    assert n % 32 != 0 and len(h) < 1_200_000
    assert_ascending_sets(h, off)
    parts = sketches(h, off)
    sizes = np.diff(off).astype(np.int64)
    assert sizes[sizes > 0].min() == pr.BOUND_MIN_REF_SIZE and np.count_nonzero(sizes == 0) == 1
    t = pr.tiles(h, off)
    at = {k: x for x, k in enumerate(t["keys"])}
    assert len(t["keys"]) == len(pairs)                              # every pair alone in its tile, no other tile
    for i, j, (kind, metric, D, s0, rule, c) in pairs:
        assert len(parts[i]) == s0 and len(parts[j]) == (c if rule == "subset" else rule) and common(parts, i, j) == c
        x = at[(i >> 5, j >> 5)]
        assert t["records"][x] == c
        if (i, j) not in (pairs[1][:2],):                            # (the one-hash sketch sits in the column block of pair 1)
            assert t["blk_min"][i >> 5] == s0 and t["blk_min"][j >> 5] == len(parts[j])
        if metric == 0:
            assert t["lb"][0][x] == s0                               # jaccard: the row's size, whatever shares the column's block
    assert t["blk_min"][pairs[0][1] >> 5] == len(parts[pairs[0][1]])    # the empty sketch is not the block's minimum
    assert t["blk_min"][pairs[1][1] >> 5] == 1
    big = [p for p in pairs if p[2][0] == "bigrow"]
    assert all(t["lb"][1][at[(i >> 5, j >> 5)]] == pr.BOUND_S and t["blk_min"][i >> 5] == 3 * pr.BOUND_S for i, j, _ in big)
    # the relation between the row bound and the first reportable count, asserted not assumed
    for D in pr.BOUND_D:
        assert pr.first_reportable(0, D, pr.BOUND_S, "subset") == pr.floor_common(0, D, pr.BOUND_S, 1) + 1
    # each pair at first_reportable is reported under its D, each one below is not; tile_stats[1] is exact
    for metric, D in pr.bound_thresholds():
        grid, rel = pr.launch_grid(t, metric, D)
        assert rel > 1e-5, (metric, D, rel)
        got = pairs_of(pr.oracle_hits(("bounds",), metric, D))
        levels, kk = pr.tile_levels(t, metric), pr.launch_kk(metric, D)
        for i, j, (kind, m, d, s0, rule, c) in pairs:
            if (m, d) == (metric, D):
                assert ((i, j) in got) == (c == pr.first_reportable(m, d, s0, rule)), (kind, m, d, c)
        for i, j in got:                                             # a required tile is launched
            assert levels[at[(i >> 5, j >> 5)]] <= kk
        assert grid == np.count_nonzero(levels <= kk)
    # the levels: kk differs by one across 2^(-k/8), and on the tight side a required tile sits on the last level covered
    for k in pr.LEVELS:
        tight, loose = pr.level_thresholds(k)
        assert (pr.launch_kk(0, tight), pr.launch_kk(0, loose)) == (k, k + 1)
        levels = pr.tile_levels(t, 0)
        got = pairs_of(pr.oracle_hits(("bounds",), 0, tight))
        assert any(levels[at[(i >> 5, j >> 5)]] == k for i, j in got), k
    assert min(pr.LEVELS) < 8 and max(pr.LEVELS) > 40 and len(pr.LEVELS) >= 4


@pytest.mark.parametrize("metric", [0, 1])
def test_sites_collections(metric):
    D = pr.SITE_D[metric]
    fc, fr = pr.site_counts(metric)
    assert fr == fc + 1                                              # (so a far genome with floor_common hashes is not reported)
    for kind in ("quiet", "edge", "loud"):
        h, off, bits = pr.sites_collection(kind, metric)
        mrs = pr.site_min_ref_size(kind, metric)
        n = len(off) - 1
        sizes = np.diff(off).astype(np.int64)
        assert n % 2 == 1 and n < 1000 and len(h) < 1_200_000 and sizes.min() == mrs
        assert math.floor(pr.min_jorc(metric, D) * mrs) >= 16      # the plan takes rk_near_kernel (RK_DIST_NEAR_MIN)
        assert_ascending_sets(h, off)
        parts = sketches(h, off)
        specs = pr.site_specs(kind, metric)
        for t, (odd, size, rels) in enumerate(specs):
            first = pr.SITE_STRIDE * t + 10
            row = first + odd
            assert len(parts[row]) == size
            for col, cnt, _ in rels:
                assert common(parts, row, first + col) == cnt
            # a site shares nothing with the other sites
            mine = np.concatenate(parts[pr.SITE_STRIDE * t:pr.SITE_STRIDE * (t + 1)])
            rest = np.concatenate(parts[:pr.SITE_STRIDE * t] + parts[pr.SITE_STRIDE * (t + 1):])
            assert len(np.intersect1d(mine, rest)) == 0
        assert common(parts, n - 2, n - 1) == fr
        for pair in (True, False):
            fb = pr.falls_back(h, off, metric, D, mrs, pair)
            if kind == "quiet":
                assert fb == []
            elif kind == "edge":                                     # one unit, with exactly floor_common far records
                t = len(specs) - 1
                assert fb == [pr.SITE_STRIDE * t + 10] and pr.far_records(h, off, fb[0], pair) == fc
            else:
                assert len(fb) >= 4
        got = pairs_of(pr.oracle_hits(("sites", kind, metric), metric, D))
        for t, (odd, size, rels) in enumerate(specs):
            first = pr.SITE_STRIDE * t + 10
            for col, cnt, _ in rels:
                assert ((first + odd, first + col) in got) == (cnt >= fr), (kind, t, col, cnt)
        assert (n - 2, n - 1) in got
    # the partner's far genome of the loud collection is 32 columns behind the partner: outside a pair's window, inside a single row's
    h, off, _ = pr.sites_collection("loud", metric)
    t = len(pr.site_specs("quiet", metric)) + 2
    first = pr.SITE_STRIDE * t + 10
    assert pr.far_records(h, off, first + 1, True) == fr and pr.far_records(h, off, first + 1, False) == 0
    # the shared slices: the first row's hashes that its partner holds too count for the partner
    first += 2 * pr.SITE_STRIDE
    assert pr.far_records(h, off, first, True) == fr == pr.far_records(h, off, first + 1, True)
    hb, offb, _ = pr.sites_collection("loud", metric, True)
    assert np.diff(offb).max() >= 65536 and len(offb) == len(off)
