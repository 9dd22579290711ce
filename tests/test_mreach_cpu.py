"""The host side of the mutual-reachability forest (rk_mreach_hits, rk_mreach_cut), the refusals of rk_mreach_rows that need no context
and the size of rk_mreach_stats -- against tests/_mreach_ref.py: the rule with exact rational ratios, sorted adjacencies and a Kruskal,
itself checked against the properties that single its result out -- and against the two oracles inside the project: rk_forest_merge
(min_pts = 1) and rk_dbscan_hits (the cut)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _dbscan_ref as dr
import _mreach_ref as mr
from rabbitkssd_amd import capi
from test_forest_cpu import records
from test_greedy_cpu import TRIPLES, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG = -1
INF = float("inf")
HITS_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
CUT_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]


def graphs(seed, count):
    """(hits, n, metric, rng) of `count` random graphs over TRIPLES (20/60 ties 25/75 under both metrics), n <= 14"""
    rng = np.random.default_rng(seed)
    for case in range(count):
        n = int(rng.integers(1, 15))
        yield random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))]), n, case % 2, rng


def compare(got, rec, n, min_pts, metric):
    """(core_dist, core_nb, edges) of the library over the records `rec` against the reference; returns the reference's (core, edges)"""
    hits = mr.hit_tuples(rec)
    dist_of = {h[:2]: float(d) for h, d in zip(hits, rec["dist"])}
    core, edges = mr.mreach(hits, n, min_pts, metric)
    core_dist, core_nb, got_edges = got
    assert core_dist.dtype == np.float64 and core_nb.dtype == np.uint32 and got_edges.dtype == capi.HIT_DTYPE
    assert core_dist.tolist() == [0.0 if min_pts == 1 else INF if c is None else dist_of[c[0][:2]] for c in core]
    assert core_nb.tolist() == [mr.NONE if c is None else c[1] for c in core]
    assert mr.hit_tuples(got_edges) == edges
    return core, edges


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_has_the_characterising_properties_on_every_small_graph():
    """every labelled graph of up to 5 vertices at every min_pts from 1 to n + 1 (python tests/_mreach_ref.py goes on to 6)"""
    assert mr.TRIPLES == TRIPLES
    seen = tied = bare = 0
    for n in range(1, 6):
        count, s, t, b = mr.exhaustive(n)
        assert count == 1 << (n * (n - 1) // 2)
        seen, tied, bare = seen + s, tied + t, bare + b
    assert seen > 10000 and tied > 3000 and bare > 10000


def test_checker_refuses_what_is_not_the_rule():
    # a path 0 - 1 - 2 - 3 whose middle pair is the nearest: at min_pts 3 the ends have no core record, 1 and 2 take their farther pair
    path = [(0, 1, 20, 50, 50), (1, 2, 60, 70, 70), (2, 3, 40, 60, 60)]
    core, edges = mr.mreach(path, 4, 3, 0)
    assert core == [None, (path[0], 0), (path[2], 3), None] and edges == [path[1]]
    mr.check_properties(path, 4, 3, 0, core, edges)
    for bad_core, bad_edges in (([None, (path[1], 2), (path[2], 3), None], edges),      # the nearest record instead of the second
                                ([(path[0], 1), (path[0], 0), (path[2], 3), None], edges),  # a core record at a genome of degree 1
                                (core, []), (core, [path[0]]), (core, [path[1], path[2]])):   # not spanning; infinite weights
        with pytest.raises(AssertionError):
            mr.check_properties(path, 4, 3, 0, bad_core, bad_edges)
    # a triangle at min_pts 2: every weight is the triangle's lightest record's ... the farthest pair (0, 2) ties nothing, the two others tie on 1's core
    tri = [(0, 1, 60, 70, 70), (0, 2, 20, 50, 50), (1, 2, 40, 60, 60)]
    core, edges = mr.mreach(tri, 3, 2, 0)
    assert [c[1] for c in core] == [1, 0, 1] and edges == [tri[0], tri[2]]
    mr.check_properties(tri, 3, 2, 0, core, edges)
    for bad in ([tri[0], tri[1]], [tri[2], tri[0]], tri):   # a heavier edge; out of order; a cycle
        with pytest.raises(AssertionError):
            mr.check_properties(tri, 3, 2, 0, core, bad)
    # at min_pts 3 all three weigh what (0, 2) weighs: (row, col) decides
    core, edges = mr.mreach(tri, 3, 3, 0)
    assert edges == [tri[0], tri[1]]
    with pytest.raises(AssertionError):
        mr.check_properties(tri, 3, 3, 0, core, [tri[0], tri[2]])
    # 25/75 = 20/60: a tie between different counts is a tie
    tie = [(0, 1, 25, 50, 50), (0, 2, 20, 40, 40), (1, 2, 20, 40, 40)]
    core, edges = mr.mreach(tie, 3, 1, 0)
    assert edges == [tie[0], tie[1]]
    with pytest.raises(AssertionError):
        mr.check_properties(tie, 3, 1, 0, core, [tie[1], tie[2]])


def test_reference_cut_is_the_dbscan_of_the_graph_below_the_threshold():
    """the first oracle, between the two references: cut where ratios above r link, the forest gives the core labels of DBSCAN over the
    hits whose ratio lies above r"""
    checked = 0
    for hits, n, metric, rng in graphs(71, 120):
        levels = sorted({mr.ratio(h, metric) for h in hits} | {0})
        for min_pts in (1, 2, 3, 5):
            core, edges = mr.mreach(hits, n, min_pts, metric)
            for r in levels:
                labels, kind, _, _ = dr.dbscan([h for h in hits if mr.ratio(h, metric) > r], n, min_pts, metric)
                assert mr.cut(edges, core, n, min_pts, metric, r) == [l if k == dr.KIND_CORE else mr.NOISE for l, k in zip(labels, kind)]
                checked += 1
    assert checked > 1000


# ---- rk_mreach_hits, rk_mreach_cut ----------------------------------------------------------------------------------------
def test_mreach_hits_equals_the_reference_the_forest_and_dbscan_on_random_graphs():
    n_edges = tied = cuts = 0
    for hits, n, metric, rng in graphs(72, 200):
        rec = records(sorted(hits), metric)
        hits = mr.hit_tuples(rec)
        top = max([sum(v in h[:2] for h in hits) for v in range(n)])   # the largest degree
        for min_pts in sorted({1, 2, 3, 4, max(1, top), top + 1, top + 2}):
            got = capi.mreach_hits(rec, n, min_pts, metric)
            core, edges = compare(got, rec, n, min_pts, metric)
            mr.check_properties(hits, n, min_pts, metric, core, edges)
            core_dist, core_nb, got_edges = got
            kept = {h[:2]: i for i, h in enumerate(hits)}
            assert all(np.array_equal(got_edges[i], rec[kept[e[:2]]]) for i, e in enumerate(edges))   # the caller's records, unchanged
            mw = [max(float(e["dist"]), core_dist[e["row"]], core_dist[e["col"]]) for e in got_edges]
            assert mw == sorted(mw)   # in doubles: the largest of three distances, ascending
            n_edges += len(edges)
            tied += sum(a == b for a, b in zip(mw, mw[1:]))
            if min_pts == 1:   # the second oracle: rk_forest_rows' forest, edge for edge
                assert np.array_equal(got_edges, capi.forest_merge(rec, rec[:0], n, metric)) and not core_dist.any()
            if min_pts == top + 2:   # above every degree: no core record, no edge
                assert len(got_edges) == 0 and np.all(np.isinf(core_dist)) and np.all(core_nb == mr.NONE)
            # the first oracle: cut at t > 0, the forest gives the core labels of rk_dbscan_hits over the records below t
            for t in sorted({1.0} | {float(d) for d in rec["dist"]} | {float(np.nextafter(d, 2.0)) for d in rec["dist"]}):
                labels, kind, _, _ = capi.dbscan_hits(rec[rec["dist"] < t], n, min_pts, metric)
                want = np.where(kind == 2, labels, np.uint32(dr.NOISE))
                assert np.array_equal(capi.mreach_cut(got_edges, core_dist, t), want), (min_pts, t)
                cuts += 1
            shuffled = rec[rng.permutation(len(rec))]   # the order of the hits does not matter
            swapped = shuffled.copy()                   # nor which endpoint is the row: sizes travel with their genome
            swapped["row"], swapped["col"], swapped["size0"], swapped["size1"] = shuffled["col"], shuffled["row"], shuffled["size1"], shuffled["size0"]
            again = capi.mreach_hits(shuffled, n, min_pts, metric)
            assert all(np.array_equal(x, y) for x, y in zip(again, got))
            other = capi.mreach_hits(swapped, n, min_pts, metric)
            back = other[2].copy()   # (the records come back as they went in: swapped)
            back["row"], back["col"], back["size0"], back["size1"] = other[2]["col"], other[2]["row"], other[2]["size1"], other[2]["size0"]
            assert np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1]) and np.array_equal(back, got_edges)
    assert n_edges > 3000 and tied > 1000 and cuts > 5000


def test_outputs_that_are_optional_and_empty_inputs():
    hits = [(0, 1, 25, 50, 50), (1, 2, 20, 40, 40), (3, 4, 60, 70, 70)]
    L = capi.lib()
    L.rk_mreach_hits.argtypes = HITS_ARGTYPES
    rec = records(hits, 0)
    core_dist = np.full(6, 77.0)
    edges, n_edges = C.c_void_p(), C.c_uint64(77)
    assert L.rk_mreach_hits(rec.ctypes.data, 3, 6, 2, 0, core_dist.ctypes.data, None, C.byref(edges), C.byref(n_edges)) == 0   # core_nb is optional
    assert n_edges.value == 3 and edges.value
    assert core_dist.tolist() == [rec["dist"][0], rec["dist"][0], rec["dist"][1], rec["dist"][2], rec["dist"][2], INF]
    assert np.array_equal(capi._take_hits(edges, n_edges), rec[[2, 0, 1]])   # 60/80, then 25/75 = 20/60 by (row, col)
    for n in (0, 1, 7):
        for min_pts, d in ((1, 0.0), (2, INF)):
            core_dist, core_nb, e = capi.mreach_hits(rec[:0], n, min_pts, 0)
            assert core_dist.tolist() == [d] * n and core_nb.tolist() == [mr.NONE] * n and len(e) == 0
            assert capi.mreach_cut(e, core_dist, 0.5).tolist() == (list(range(n)) if min_pts == 1 else [dr.NOISE] * n)
    assert L.rk_mreach_hits(None, 0, 0, 1, 0, None, None, C.byref(edges), C.byref(n_edges)) == 0 and n_edges.value == 0   # no genome: nothing to write
    L.rk_free_host.argtypes = [C.c_void_p]
    L.rk_free_host(edges)
    L.rk_mreach_cut.argtypes = CUT_ARGTYPES
    assert L.rk_mreach_cut(None, 0, None, 0, 0.5, None) == 0
    # a record without a ratio (metric 0: u = 4 + 4 - 10 < 0) weighs more than every record that has one, and is no infinite weight
    odd = records([(0, 1, 60, 70, 70), (0, 2, 10, 4, 4), (1, 2, 1, 50, 50)], 0)
    core_dist, core_nb, e = capi.mreach_hits(odd, 3, 1, 0)
    assert mr.hit_tuples(e) == mr.hit_tuples(odd[[0, 2]])
    core_dist, core_nb, e = capi.mreach_hits(odd, 3, 3, 0)
    assert core_nb.tolist() == [2, 2, 0] and mr.hit_tuples(e) == mr.hit_tuples(odd[[0, 1]])   # every weight is that record's: (row, col) decides


def test_mreach_hits_and_cut_refusals_write_nothing():
    L = capi.lib()
    L.rk_mreach_hits.argtypes = HITS_ARGTYPES
    L.rk_mreach_cut.argtypes = CUT_ARGTYPES
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)], 0)
    core_dist, core_nb, labels = np.full(4, 77.0), np.full(4, 77, dtype=np.uint32), np.full(4, 77, dtype=np.uint32)
    edges, n_edges = C.c_void_p(77), C.c_uint64(77)
    out = (core_dist.ctypes.data, core_nb.ctypes.data, C.byref(edges), C.byref(n_edges))
    for bad in ([(0, 4, 25, 50, 50)], [(4, 5, 25, 50, 50)], [(1, 0xFFFFFFFF, 25, 50, 50)], [(2, 2, 25, 50, 50)]):
        both = np.concatenate([good, records(bad, 0)])
        assert L.rk_mreach_hits(both.ctypes.data, 3, 4, 2, 0, *out) == RK_ERR_ARG
        with pytest.raises(capi.RkError) as e:
            capi.mreach_hits(both, 4, 2, 0)
        assert e.value.code == RK_ERR_ARG
        if bad[0][0] != bad[0][1]:
            assert L.rk_mreach_cut(both.ctypes.data, 3, core_dist.ctypes.data, 4, 0.5, labels.ctypes.data) == RK_ERR_ARG
            with pytest.raises(capi.RkError) as e:
                capi.mreach_cut(both, core_dist, 0.5)
            assert e.value.code == RK_ERR_ARG
    assert L.rk_mreach_hits(good.ctypes.data, 2, 4, 0, 0, *out) == RK_ERR_ARG   # min_pts counts the genome itself
    assert L.rk_mreach_hits(None, 2, 4, 2, 0, *out) == RK_ERR_ARG
    assert L.rk_mreach_hits(good.ctypes.data, 2, 4, 2, 0, None, out[1], out[2], out[3]) == RK_ERR_ARG
    assert L.rk_mreach_hits(good.ctypes.data, 2, 4, 2, 0, out[0], out[1], None, out[3]) == RK_ERR_ARG
    assert L.rk_mreach_hits(good.ctypes.data, 2, 4, 2, 0, out[0], out[1], out[2], None) == RK_ERR_ARG
    assert L.rk_mreach_cut(None, 2, core_dist.ctypes.data, 4, 0.5, labels.ctypes.data) == RK_ERR_ARG
    assert L.rk_mreach_cut(good.ctypes.data, 2, None, 4, 0.5, labels.ctypes.data) == RK_ERR_ARG
    assert L.rk_mreach_cut(good.ctypes.data, 2, core_dist.ctypes.data, 4, 0.5, None) == RK_ERR_ARG
    assert np.all(core_dist == 77.0) and np.all(core_nb == 77) and np.all(labels == 77) and edges.value == 77 and n_edges.value == 77


def test_cut_is_strict_and_labels_by_the_smallest_core_genome():
    # 0 - 1 - 2 - 3 - 4, the middle pairs nearer: at min_pts 3 genome 0 and 4 have no core record; 1, 2, 3 link at their farther pairs
    rec = records([(0, 1, 20, 50, 50), (1, 2, 60, 70, 70), (2, 3, 60, 70, 70), (3, 4, 40, 60, 60)], 0)
    core_dist, core_nb, edges = capi.mreach_hits(rec, 5, 3, 0)
    d = rec["dist"]
    assert d[0] > d[3] > d[1] == d[2]
    assert core_dist.tolist() == [INF, d[0], d[1], d[3], INF] and core_nb.tolist() == [mr.NONE, 0, 3, 4, mr.NONE]
    assert mr.hit_tuples(edges) == mr.hit_tuples(rec[[2, 1]])   # (2, 3) weighs d[3], (1, 2) weighs d[0]
    N = dr.NOISE
    for t, want in ((d[1], [N] * 5), (float(np.nextafter(d[1], 1.0)), [N, N, 2, N, N]), (d[3], [N, N, 2, N, N]),
                    (float(np.nextafter(d[3], 1.0)), [N, N, 2, 2, N]), (d[0], [N, N, 2, 2, N]), (float(np.nextafter(d[0], 1.0)), [N, 1, 1, 1, N]),
                    (1.0, [N, 1, 1, 1, N])):
        assert capi.mreach_cut(edges, core_dist, t).tolist() == want, t


# ---- what needs no context ------------------------------------------------------------------------------------------------
def test_mreach_rows_refuses_null_arguments_and_the_symbols_are_exported():
    L = capi.lib()
    L.rk_mreach_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64), C.POINTER(capi.MreachStats)]
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    assert L.rk_mreach_rows(None, None, C.byref(opts), 3, None, None, None, None, None) == RK_ERR_ARG
    assert L.rk_mreach_rows(None, None, None, 3, None, None, None, None, None) == RK_ERR_ARG
    for name in ("rk_mreach_rows", "rk_mreach_hits", "rk_mreach_cut"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.mreach_rows) and callable(capi.mreach_hits) and callable(capi.mreach_cut)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_MREACH 10\b", hdr)
    assert re.search(r"#define RK_MREACH_NONE 0xFFFFFFFFu\b", hdr) and capi.MREACH_NONE == mr.NONE == 0xFFFFFFFF
    assert L.rk_ctx_last_ms(None, 10) == 0.0 and math.isinf(INF)


def test_mreach_stats_has_the_headers_size():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    m = re.search(r"typedef struct rk_mreach_stats \{(.*?)\} rk_mreach_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    width = {"uint64_t": 8, "uint32_t": 4}
    fields = [(t, name) for t, name in re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [name for _, name in fields] == [name for name, _ in capi.MreachStats._fields_]
    assert [name for _, name in fields] == ["edges", "borderline", "borderline_kept", "join_attempts", "border_attempts", "rounds", "n_trees", "n_core",
                                            "max_degree", "path", "pad_"]
    assert C.sizeof(capi.MreachStats) == sum(width[t] for t, _ in fields) == 56
    for (t, name), (_, ctype) in zip(fields, capi.MreachStats._fields_):
        assert C.sizeof(ctype) == width[t], name
