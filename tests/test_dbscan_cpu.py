"""The host side of the density-based clusters (rk_dbscan_hits), the refusals of rk_dbscan_rows that need no context and the size of
rk_dbscan_stats -- against tests/_dbscan_ref.py: the rule with exact rational ratios, adjacency sets and a breadth-first search, itself
checked against the properties that single its result out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _dbscan_ref as dr
from _selfjoin_cases import labels_of
from rabbitkssd_amd import capi
from test_greedy_cpu import TRIPLES, random_graph, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG = -1
HITS_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.POINTER(capi.DbscanStats)]


def graphs(seed, count):
    """(hits, n, metric, rng) of `count` random graphs over TRIPLES (20/60 ties 25/75 under both metrics), n <= 14"""
    rng = np.random.default_rng(seed)
    for case in range(count):
        n = int(rng.integers(1, 15))
        yield random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))]), n, case % 2, rng


def compare(got, hits, n, min_pts, metric):
    """(labels, kind, via, degree) of the library against the reference; returns the reference's"""
    want = dr.dbscan(hits, n, min_pts, metric)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint8 and got[2].dtype == np.uint32 and got[3].dtype == np.uint32
    for mine, ref, what in zip(got, want, ("labels", "kind", "via", "degree")):
        assert mine.tolist() == ref, what
    return want


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_has_the_characterising_properties_on_every_small_graph():
    """Every graph of up to 5 vertices at every min_pts; of the 2^15 graphs of 6 vertices every 16th, of the 2^21 of 7 every 2039th
    (each check costs ~0.1 ms here: all of them take half an hour -- python tests/_dbscan_ref.py runs them)"""
    assert dr.TRIPLES == TRIPLES
    borders = ties = 0
    for n, stride in ((1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 16), (7, 2039)):
        count, b, t = dr.exhaustive(n, stride, first=n % stride)
        assert count == -(-((1 << (n * (n - 1) // 2)) - n % stride) // stride)
        borders += b
        ties += t
    assert borders > 10000 and ties > 500


def test_checker_refuses_what_is_not_the_rule():
    # a path 0 - 1 - 2 - 3 - 4 at min_pts 3: the interior is core, the ends are border
    path = [(i, i + 1, 25, 50, 50) for i in range(4)]
    good = dr.dbscan(path, 5, 3, 0)
    assert good == ([1, 1, 1, 1, 1], [1, 2, 2, 2, 1], [1, dr.NOISE, dr.NOISE, dr.NOISE, 3], [1, 2, 2, 2, 1])
    dr.check_properties(path, 5, 3, 0, *good)
    for at, wrong in ((0, [0, 1, 1, 1, 1]), (0, [1, 1, 3, 3, 1]), (1, [2, 2, 2, 2, 1]), (1, [0, 2, 2, 2, 1]), (2, [3, dr.NOISE, dr.NOISE, dr.NOISE, 3]),
                      (3, [1, 2, 2, 2, 2])):   # the smallest member instead of the smallest core; a split cluster; kinds; a via that is not adjacent; a degree
        bad = list(good)
        bad[at] = wrong
        with pytest.raises(AssertionError):
            dr.check_properties(path, 5, 3, 0, *bad)
    # x = 2 between the cores 0 and 1 (each made core at min_pts 4 by two satellites): the nearer one, and at a tie the smaller index
    sat = [(0, 3, 60, 70, 70), (0, 4, 60, 70, 70), (1, 5, 60, 70, 70), (1, 6, 60, 70, 70)]
    fork = sat + [(0, 2, 20, 50, 50), (1, 2, 40, 60, 60)]
    labels, kind, via, degree = dr.dbscan(fork, 7, 4, 0)
    assert (labels[2], kind[2], via[2]) == (1, 1, 1) and labels[:2] == [0, 1]
    with pytest.raises(AssertionError):
        dr.check_properties(fork, 7, 4, 0, [0, 1, 0, 0, 0, 1, 1], kind, [dr.NOISE, dr.NOISE, 0, 0, 0, 1, 1], degree)
    for a, b in (((0, 2, 25, 70, 30), (1, 2, 20, 50, 30)), ((0, 2, 20, 50, 30), (1, 2, 25, 70, 30))):   # 25/75 = 20/60
        tie = sat + [b, a]
        labels, kind, via, degree = dr.dbscan(tie, 7, 4, 0)
        assert (labels[2], kind[2], via[2]) == (0, 1, 0)
        with pytest.raises(AssertionError):
            dr.check_properties(tie, 7, 4, 0, [0, 1, 1, 0, 0, 1, 1], kind, [dr.NOISE, dr.NOISE, 1, 0, 0, 1, 1], degree)
    with pytest.raises(AssertionError):   # a noise genome next to a core one
        dr.check_properties(path, 5, 3, 0, [dr.NOISE, 1, 1, 1, 1], [0, 2, 2, 2, 1], [dr.NOISE] * 4 + [3], [1, 2, 2, 2, 1])


# ---- rk_dbscan_hits -------------------------------------------------------------------------------------------------------
def test_dbscan_hits_equals_the_reference_on_random_graphs():
    borders = ties = 0
    for hits, n, metric, rng in graphs(70, 200):
        rec = records(hits)
        top = max(sum(v in h[:2] for h in hits) for v in range(n))   # the largest degree
        for min_pts in sorted({1, 2, 3, 4, max(1, top), top + 1, top + 2}):
            got = capi.dbscan_hits(rec, n, min_pts, metric)
            want = compare(got, hits, n, min_pts, metric)
            dr.check_properties(hits, n, min_pts, metric, *got)
            borders += want[1].count(dr.KIND_BORDER)
            if min_pts == 1:   # every genome core: single linkage
                assert got[0].tolist() == labels_of([h[:2] for h in hits], n).tolist() and set(got[1].tolist()) == {2}
            if min_pts == 2:   # single linkage, isolated genomes as noise
                single = labels_of([h[:2] for h in hits], n).tolist()
                assert got[0].tolist() == [dr.NOISE if want[3][v] == 0 else single[v] for v in range(n)] and 1 not in got[1].tolist()
            if min_pts == top + 2:   # above every degree: all noise
                assert got[0].tolist() == [dr.NOISE] * n == got[2].tolist() and not got[1].any()
            shuffled = rec[rng.permutation(len(rec))]   # the order of the hits does not matter
            swapped = shuffled.copy()                   # nor which endpoint is the row: sizes travel with their genome
            swapped["row"], swapped["col"], swapped["size0"], swapped["size1"] = shuffled["col"], shuffled["row"], shuffled["size1"], shuffled["size0"]
            for again in (capi.dbscan_hits(shuffled, n, min_pts, metric), capi.dbscan_hits(swapped, n, min_pts, metric)):
                assert all(np.array_equal(x, y) for x, y in zip(again, got))
        ties += sum(h[2:] in (TRIPLES[3], TRIPLES[4]) for h in hits)
    assert borders > 1000 and ties > 300


def test_outputs_that_are_optional_and_empty_inputs():
    hits = [(0, 1, 25, 50, 50), (1, 2, 20, 40, 40), (3, 4, 60, 70, 70)]
    L = capi.lib()
    L.rk_dbscan_hits.argtypes = HITS_ARGTYPES
    rec = records(hits)
    labels, kind = np.full(6, 77, dtype=np.uint32), np.full(6, 77, dtype=np.uint8)
    assert L.rk_dbscan_hits(rec.ctypes.data, 3, 6, 3, 0, labels.ctypes.data, kind.ctypes.data, None, None) == 0   # via and degree are optional
    assert labels.tolist() == [1, 1, 1] + [dr.NOISE] * 3 and kind.tolist() == [1, 2, 1, 0, 0, 0]
    for n in (0, 1, 7):
        got = capi.dbscan_hits(records([]), n, 1, 0)
        assert got[0].tolist() == list(range(n)) and got[1].tolist() == [2] * n and got[2].tolist() == [dr.NOISE] * n and got[3].tolist() == [0] * n
        got = capi.dbscan_hits(records([]), n, 2, 0)
        assert got[0].tolist() == [dr.NOISE] * n and not got[1].any()
    assert L.rk_dbscan_hits(None, 0, 6, 1, 0, labels.ctypes.data, kind.ctypes.data, None, None) == 0   # a list of no hits may be NULL
    assert labels.tolist() == list(range(6))
    assert L.rk_dbscan_hits(None, 0, 0, 1, 0, None, None, None, None) == 0   # no genome: nothing to write
    # a record without a ratio (metric 0: u = 4 + 4 - 10 < 0) comes behind every record that has one
    odd = [(0, 1, 60, 70, 70), (0, 2, 60, 70, 70), (3, 4, 60, 70, 70), (3, 5, 60, 70, 70), (0, 6, 10, 4, 4), (3, 6, 1, 50, 50)]
    got = capi.dbscan_hits(records(odd), 7, 4, 0)
    compare(got, odd, 7, 4, 0)
    assert got[1].tolist() == [2, 1, 1, 2, 1, 1, 1] and got[2][6] == 3


def test_dbscan_hits_refusals_write_nothing():
    L = capi.lib()
    L.rk_dbscan_hits.argtypes = HITS_ARGTYPES
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)])
    labels, via, degree = (np.full(4, 77, dtype=np.uint32) for _ in range(3))
    kind = np.full(4, 77, dtype=np.uint8)
    out = (labels.ctypes.data, kind.ctypes.data, via.ctypes.data, degree.ctypes.data)
    for bad in ([(0, 4, 25, 50, 50)], [(4, 5, 25, 50, 50)], [(1, 0xFFFFFFFF, 25, 50, 50)], [(2, 2, 25, 50, 50)]):
        both = np.concatenate([good, records(bad)])
        assert L.rk_dbscan_hits(both.ctypes.data, 3, 4, 2, 0, *out) == RK_ERR_ARG
        with pytest.raises(capi.RkError) as e:
            capi.dbscan_hits(both, 4, 2, 0)
        assert e.value.code == RK_ERR_ARG
    assert L.rk_dbscan_hits(good.ctypes.data, 2, 4, 0, 0, *out) == RK_ERR_ARG   # min_pts counts the genome itself
    assert L.rk_dbscan_hits(None, 2, 4, 2, 0, *out) == RK_ERR_ARG
    assert L.rk_dbscan_hits(good.ctypes.data, 2, 4, 2, 0, None, out[1], out[2], out[3]) == RK_ERR_ARG
    assert L.rk_dbscan_hits(good.ctypes.data, 2, 4, 2, 0, out[0], None, out[2], out[3]) == RK_ERR_ARG
    assert all(np.all(a == 77) for a in (labels, kind, via, degree))   # refused before anything is written
    assert L.rk_dbscan_hits(good.ctypes.data, 2, 4, 2, 0, *out) == 0
    assert labels.tolist() == [0, 0, 2, 2] and kind.tolist() == [2] * 4 and via.tolist() == [dr.NOISE] * 4 and degree.tolist() == [1] * 4


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_dbscan_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_dbscan_rows.argtypes = ROWS_ARGTYPES
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    labels, kind, st = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint8), capi.DbscanStats()
    assert L.rk_dbscan_rows(None, None, C.byref(opts), 3, labels.ctypes.data, kind.ctypes.data, None, None, C.byref(st)) == RK_ERR_ARG
    assert L.rk_dbscan_rows(None, None, None, 3, None, None, None, None, None) == RK_ERR_ARG


def test_dbscan_symbols_are_exported():
    L = capi.lib()
    for name in ("rk_dbscan_rows", "rk_dbscan_hits"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.dbscan_rows) and callable(capi.dbscan_hits)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_DBSCAN 9\b", hdr)
    assert re.search(r"#define RK_DBSCAN_NOISE 0xFFFFFFFFu\b", hdr) and capi.DBSCAN_NOISE == dr.NOISE == 0xFFFFFFFF
    assert capi.DBSCAN_KINDS == dr.KIND_NAMES


def test_dbscan_stats_has_the_headers_size():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    m = re.search(r"typedef struct rk_dbscan_stats \{(.*?)\} rk_dbscan_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    width = {"uint64_t": 8, "uint32_t": 4}
    fields = [(t, name) for t, name in re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [name for _, name in fields] == [name for name, _ in capi.DbscanStats._fields_]
    assert [name for _, name in fields] == ["edges", "borderline", "borderline_kept", "join_attempts", "border_attempts", "n_clusters", "n_core", "n_border",
                                            "n_noise"]
    assert C.sizeof(capi.DbscanStats) == sum(width[t] for t, _ in fields) == 48
    for (t, name), (_, ctype) in zip(fields, capi.DbscanStats._fields_):
        assert C.sizeof(ctype) == width[t], name
