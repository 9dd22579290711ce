"""The model and the generators of tests/_rows_ref.py, checked on the CPU before a GPU is involved: the slice totals against a
brute force over two tiny hand-written collections, `common_matrix`, the bookkeeping of `candidates` and the designated cells
against the oracle, the list events on hand-made runs, and every "the seam is present" condition the legs of tests/test_gpu_rows_edges.py rest on (they assert them
again)."""
import numpy as np
import pytest

from oracle import oracle as ok

import _prune_ref as pr
import _rows_ref as rr


def tiny(sketches):
    return rr.csr([np.array(s, dtype=np.uint32) for s in sketches])


# 40 genomes: hash 5 in a pair and later (covered for 1), 6 in a pair only, 7 spans 39 ids (a range), 8 for the partner alone,
# 9 in (2, 3) and 3's open slice 11
TINY_SETS = [[5, 6, 7], [5, 6, 8], [9, 5], [9, 11, 8], [11], [7]] + [[100 + g] for g in range(6, 39)] + [[7, 5]]
# genome 1 repeats hash 5 (its copies follow each other in the list), genome 3 repeats 9
TINY_MULTI = [[5, 7], [5, 5, 8], [9, 5], [9, 9, 8], [9], [7]]


@pytest.mark.parametrize("sketches,sets", [(TINY_SETS, True), (TINY_MULTI, False)], ids=["sets", "multiset"])
def test_slice_totals_against_brute_force(sketches, sets):
    h, off = tiny(sketches)
    s = rr.slices(h, off)
    assert s["sets"] == sets
    assert rr.slice_totals(s) == rr.brute_force_totals(h, off)
    assert (rr.slice_totals(s)[1] == 0) == (not sets)
    # the postings are the oracle's, every record's holders are later ones (or the genome's own repeats)
    postings, _ = ok.index_build32(h, off, 8)
    assert np.array_equal(s["postings"], postings)
    for r in s["rec"]:
        later = s["postings"][r["lo"]:r["hi"]]
        assert later[0] == r["first"] and later[-1] == r["last"] and np.all(later >= r["g"]) and np.all(np.diff(later) >= 0)


def test_tiny_collection_by_hand():
    h, off = tiny(TINY_SETS)
    s = rr.slices(h, off)
    # hash 5: holders 0 1 2 39 -> three records (1's is covered); 6: one; 7: 0 -> (5, 39): two records, the first a range;
    # 8: 1 -> 3; 9: 2 -> 3; 11: 3 -> 4
    assert rr.slice_totals(s) == (3 + 1 + 2 + 1 + 1 + 1, 3 + 1 + 1 + 1 + 1 + 1 - 2, 8)
    u = rr.unit_classes(s, 0, True, 256)
    # the pair (0, 1): 5 is shared (first holder is the partner) and a range (last - first = 38), 6 is the partner alone in
    # the window, 7 a range of two; then the partner's open slice of 8
    assert [(int(x["form"]), bool(x["shared"]), bool(x["in_b"])) for x in u] == [(rr.SHORT, True, False), (rr.WINDOW, True, False), (rr.SHORT, False, False), (rr.WINDOW, False, True)]
    assert len(rr.unit_classes(s, 1, False, 256)) == 2       # a single row walks its covered slice too


def test_list_events_by_hand():
    assert rr.list_events([255, 256, 257], 256, False) == [("fits", 255), ("fits", 256), ("overflow", 0, 257)]
    assert rr.list_events([127, 1, 5], 256, True) == [("wait", 127), ("flush", 128), ("wait", 5), ("final", 5)]
    assert rr.list_events([127, 130, 126, 130], 256, True) == [("wait", 127), ("overflow", 127, 130), ("wait", 126), ("flush", 256), ("final", 0)]
    assert rr.run_events(np.array([1, 2, 3]), 16, True, 2) == [[("wait", 1), ("wait", 3), ("final", 3)], [("wait", 3), ("final", 3)]]


@pytest.mark.parametrize("multiset", [False, True])
def test_forms_collection(multiset):
    h, off, bits, want = rr.forms_collection(multiset)
    for g in range(len(off) - 1):
        x = h[int(off[g]):int(off[g + 1])]
        assert np.all(x[1:] > x[:-1]) or (multiset and g == 200 and np.all(x[1:] >= x[:-1]))
    assert h.max() < 1 << bits
    for pair in (True, False):
        if multiset and pair:
            continue
        for threads in (256, 512, 1024):
            totals = rr.forms_conditions(multiset, pair, threads)
    assert totals == rr.slice_totals(rr.slices(h, off))
    # the designated cells: the generator's count is the oracle's `common`, under the loose threshold and in the dense report
    for D in (rr.FORMS_D, 1.5):
        cells = rr.hit_cells(rr.oracle_hits(("forms", multiset), 1, D))
        assert all(cells.get(k) == v for k, v in want.items()) and len(want) > 600
    n = len(off) - 1
    assert len(rr.oracle_hits(("forms", multiset), 1, 1.5)) == n * (n - 1) // 2
    if not multiset:
        m = rr.common_matrix(h, off)
        assert all(m[k] == v for k, v in want.items())
        for r in set(k[0] for k in want):       # and they are all the non-zero cells of their rows
            assert {(r, r + 1 + int(c)) for c in np.flatnonzero(m[r, r + 1:])} == {k for k in want if k[0] == r}


def test_candidates_against_the_oracles_dense_matrix():
    """common_matrix against the oracle's dense counts, and the bookkeeping of candidates() per unit and tile recomputed from
    them (the bound itself is min_common in both: that the designed rows' cells ARE reportable rests on lists_conditions, which
    counts the oracle's hits per row)"""
    h, off, bits = rr.lists_collection()
    sizes = np.diff(off).astype(np.int64)
    postings, counts = ok.index_build32(h, off, bits)
    _, dense = ok.index_dist32(counts, bits, postings, sizes.astype(np.uint32), h, off, 1, 1, rr.K, rr.LISTS_D, threads=8, want_dense=True)
    m = rr.common_matrix(h, off)
    assert np.array_equal(np.triu(dense, 1), np.triu(m, 1))
    mrs = int(sizes[sizes > 0].min())
    for unit_rows, tile_cols in ((1, None), (2, None), (1, 512)):
        c = rr.candidates(m, sizes, 1, rr.LISTS_D, unit_rows=unit_rows, tile_cols=tile_cols)
        tc = tile_cols or len(sizes)
        for unit in (0, 5, 14, 40, 63, 70, 200, 500):
            want = np.zeros(c.shape[1], dtype=np.int64)
            for r in range(unit * unit_rows, min(len(sizes), (unit + 1) * unit_rows)):
                cols = np.arange(r + 1, len(sizes))
                cols = cols[dense[r, r + 1:] >= rr.min_common(1, rr.LISTS_D, int(sizes[r]), mrs)]
                want += np.bincount(cols // tc, minlength=c.shape[1])
            assert np.array_equal(c[unit], want), (unit_rows, tile_cols, unit)


@pytest.mark.parametrize("cap", rr.LISTS_CAPS)
def test_lists_collection(cap):
    for kind in ("single", "pairs", "tiles"):
        rr.lists_conditions(cap, kind)
    assert rr.tile_cols_of(rr.LISTS_N, 2) == 512


@pytest.mark.parametrize("big,repeat", [(65535, False), (65536, False), (65535, True)])
def test_width_collection(big, repeat):
    h, off, bits = rr.width_collection(big, repeat)
    sizes = np.diff(off)
    assert sizes.max() == big + repeat and len(sizes) < 40
    s = rr.slices(h, off)
    assert s["sets"] == (not repeat)
    a, b, c = rr.WIDTH_BIG
    assert b % 2 == 1 and c % 2 == 0                      # the high and the low half of an LDS word
    cells = rr.hit_cells(rr.oracle_hits(("width", big, repeat), 1, 0.1))
    assert cells[(a, c)] == big and cells[(b, c)] == big + repeat and cells[(a, b)] == big + repeat
    assert cells[(a, b - 1)] == 3 and cells[(a, c + 1)] == 3           # the other halves of those words are not zero


def test_queues_collection():
    grid, totals = rr.queues_conditions(24)
    assert grid == 1152 and totals[2] <= totals[0]


@pytest.mark.parametrize("metric", [0, 1])
def test_far_family_falls_back_and_overflows_a_list_of_16(metric):
    h, off, _ = pr.sites_collection("family", metric)
    D, mrs = pr.SITE_D[metric], pr.site_min_ref_size("family", metric)
    sizes = np.diff(off).astype(np.int64)
    n = len(sizes)
    assert sizes.min() == mrs and 512 < n <= 1024
    fb = pr.falls_back(h, off, metric, D, mrs, True)
    assert set(pr.falls_back(*pr.sites_collection("loud", metric)[:2], metric, D, mrs, True)) < set(fb)
    cells = rr.candidates(rr.common_matrix(h, off), sizes, metric, D, tile_cols=rr.tile_cols_of(n, 2))
    assert [r for r in fb if cells[r].max() > 16] == [fb[-1]] and cells[fb[-1]].max() == pr.FAMILY
    got = set(zip(*[pr.oracle_hits(("sites", "family", metric), metric, D)[f].tolist() for f in ("row", "col")]))
    assert {(fb[-1], fb[-1] + 33 + i) for i in range(pr.FAMILY)} <= got


def test_bands_pairs_lie_on_either_side_of_every_boundary():
    band_rows, edges = [912, 2496], [(0, 1536), (912, 2432)]
    pairs = rr.bands_pairs(2999, band_rows, edges)
    for b in band_rows:
        assert {(b - 2, b + 1), (b - 1, b), (b - 1, b + 2), (b, b + 1)} <= set(pairs)     # across, both rows of a pair, and behind
    for r, c in edges:
        assert {(r, c - 1), (r, c), (r + 1, c - 1), (r + 1, c)} <= set(pairs)
    h, off, bits = rr.bands_collection(2999, pairs)
    want = rr.dist_hits(h, off, bits, 1, rr.BANDS_D)
    assert set(zip(want["row"].tolist(), want["col"].tolist())) == set(pairs) and np.all(want["common"] == 3)
