"""The host side of the k nearest neighbours (rk_knn_hits, rk_knn_merge), the refusals of rk_knn_rows that need no context and the
size of rk_knn_stats -- against tests/_knn_ref.py: per genome the first k incident records with exact rational ratios, itself checked
against the properties that single its result out, and its model of the selection wave of rk_knn.hip, checked against that
reference over adversarial streams."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _knn_ref as kr
from rabbitkssd_amd import capi
from test_greedy_cpu import TRIPLES, random_graph, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG = -1
HITS_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
MERGE_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                  C.POINTER(C.c_uint64)]


def graphs(seed, count):
    """(hits, n, metric) of `count` random graphs over TRIPLES (20/60 ties 25/75 under both metrics), n <= 14"""
    rng = np.random.default_rng(seed)
    for case in range(count):
        n = int(rng.integers(1, 15))
        yield random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))]), n, case % 2, rng


def compare(got, hits, n, k, metric):
    """(off, nbrs) of the library against the reference; returns the reference's lists"""
    off, nbrs = got
    want = kr.knn(hits, n, k, metric)
    assert off.dtype == np.uint64 and off.tolist() == kr.offsets(want)
    assert kr.hit_tuples(nbrs) == kr.flat(want)
    return want


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_has_the_characterising_properties():
    ties = 0
    for hits, n, metric, _ in graphs(60, 300):
        for k in (1, 2, 3, n):
            lists = kr.knn(hits, n, k, metric)
            kr.check_properties(hits, n, k, metric, lists)
            assert kr.offsets(lists)[-1] == sum(min(k, sum(v in h[:2] for h in hits)) for v in range(n))
        ties += sum(h[2:] in (TRIPLES[3], TRIPLES[4]) for h in hits)
    assert ties > 300
    # the checker does refuse: the farther neighbour, the larger index of a tie, a list that is too short, a record of another genome
    fork = [(0, 1, 20, 50, 50), (0, 2, 40, 60, 60), (1, 2, 60, 70, 70)]
    assert kr.knn(fork, 3, 1, 0) == [[fork[1]], [fork[2]], [fork[2]]]
    with pytest.raises(AssertionError):
        kr.check_properties(fork, 3, 1, 0, [[fork[0]], [fork[2]], [fork[2]]])
    tie = [(0, 1, 25, 50, 50), (0, 2, 20, 40, 40)]   # 25/75 = 20/60: the smaller neighbour wins
    assert kr.knn(tie, 3, 1, 0)[0] == [tie[0]] and kr.knn(tie, 3, 1, 1)[0] == [tie[0]]
    with pytest.raises(AssertionError):
        kr.check_properties(tie, 3, 1, 0, [[tie[1]], [tie[0]], [tie[1]]])
    with pytest.raises(AssertionError):
        kr.check_properties(fork, 3, 2, 0, [[fork[1]], [fork[2], fork[0]], [fork[2], fork[1]]])
    with pytest.raises(AssertionError):
        kr.check_properties(fork, 3, 1, 0, [[fork[2]], [fork[2]], [fork[2]]])
    with pytest.raises(AssertionError):   # in the wrong order
        kr.check_properties(fork, 3, 2, 0, [[fork[0], fork[1]], [fork[2], fork[0]], [fork[2], fork[1]]])


# ---- the model of the wave ----------------------------------------------------------------------------------------------
def star(degree, metric, pattern, rng):
    """records of hub 0 with `degree` leaves, in stream order, the leaves' indices shuffled against it"""
    leaves = (rng.permutation(degree) + 1).tolist()
    hits = []
    for at, leaf in enumerate(leaves):
        if pattern == "nearest_last":
            triple = (at + 1, 200, 200)
        elif pattern == "nearest_first":
            triple = (degree - at, 200, 200)
        elif pattern == "all_ties":
            triple = ((20, 50, 30), (25, 70, 30))[at % 2] if metric == 0 else ((20, 40, 70), (25, 50, 60))[at % 2]
        else:   # ties across the seam between two chunks: the best ratio at stream places 60 .. 68, from two different counts
            tied = at % 64 >= 60 or at % 64 < 5
            triple = ((100, 250, 150), (120, 300, 180))[at % 2] if tied else (1 + at % 7, 200, 200)
            if metric == 1:
                triple = ((100, 200, 300), (120, 240, 250))[at % 2] if tied else triple
        hits.append((0, leaf) + triple)
    return hits


@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_selection_model_equals_the_reference_over_adversarial_streams(k):
    rng = np.random.default_rng(61)
    inserted_late = 0
    for degree in sorted({0, 1, max(0, k - 1), k, k + 1, 63, 64, 65, 128, 129}):
        for metric in (0, 1):
            for pattern in ("nearest_last", "nearest_first", "all_ties", "seam_ties"):
                hits = star(degree, metric, pattern, rng)
                entries = [kr.entry(h, 0, e, metric) for e, h in enumerate(hits)]
                got = kr.select_model(entries, k)
                want = kr.knn(hits, degree + 1, k, metric)[0]
                assert [hits[x & 0xFFFFFFFF] for _, x in got] == want, (degree, metric, pattern)
                assert got == sorted(entries)[:k]   # entries compared as (first word, second word) are the order
                if pattern == "nearest_last" and degree > k:
                    inserted_late += hits.index(want[0]) == degree - 1
    assert inserted_late == 2 * sum(d > k for d in {0, 1, max(0, k - 1), k, k + 1, 63, 64, 65, 128, 129})


def test_selection_model_on_random_streams_with_equal_ratios_from_different_counts():
    rng = np.random.default_rng(62)
    for case in range(60):
        degree, k, metric = int(rng.integers(0, 200)), int(rng.integers(1, 65)), case % 2
        leaves = (rng.permutation(degree) + 1).tolist()
        hits = [(0, leaf) + TRIPLES[int(rng.integers(len(TRIPLES)))] for leaf in leaves]
        entries = [kr.entry(h, 0, e, metric) for e, h in enumerate(hits)]
        assert [hits[x & 0xFFFFFFFF] for _, x in kr.select_model(entries, k)] == kr.knn(hits, degree + 1, k, metric)[0]


# ---- rk_knn_hits ----------------------------------------------------------------------------------------------------------
def test_knn_hits_equals_the_reference_on_random_graphs():
    returned = 0
    for hits, n, metric, rng in graphs(63, 300):
        rec = records(hits)
        by_pair = {(int(r["row"]), int(r["col"])): r for r in rec}
        for k in (1, 2, 3, n, 1000):   # (1000: larger than every degree)
            got = capi.knn_hits(rec, n, k, metric)
            want = compare(got, hits, n, k, metric)
            kr.check_properties(hits, n, k, metric, [kr.hit_tuples(got[1][int(got[0][v]): int(got[0][v + 1])]) for v in range(n)])
            returned += len(got[1])
            for r in got[1]:   # the records travel unchanged, marks included
                assert r == by_pair[(int(r["row"]), int(r["col"]))]
            if k == 1000:
                assert len(got[1]) == 2 * len(hits)
            again = capi.knn_hits(rec[rng.permutation(len(rec))], n, k, metric)   # the order of the hits does not matter
            assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
            assert all(len(want[v]) == 0 for v in range(n) if not any(v in h[:2] for h in hits))   # an isolated genome
    assert returned > 5000


def test_records_without_a_ratio_sort_last_and_empty_inputs():
    # metric 0: u = 4 + 4 - 10 < 0 and common < 0 have no ratio; among themselves the neighbour's index decides
    hits = [(0, 1, 10, 4, 4), (0, 2, -1, 5, 5), (0, 3, 1, 50, 50), (0, 4, 20, 50, 50), (1, 4, 3, 50, 50)]
    for k in (1, 2, 3, 4, 5):
        off, nbrs = capi.knn_hits(records(hits), 5, k, 0)
        compare((off, nbrs), hits, 5, k, 0)
        assert kr.hit_tuples(nbrs[: min(k, 4)]) == [hits[3], hits[2], hits[0], hits[1]][:k]
    compare(capi.knn_hits(records(hits), 5, 4, 1), hits, 5, 4, 1)   # (metric 1: 10/4 is a ratio, the largest)
    for n in (0, 1, 7):
        off, nbrs = capi.knn_hits(records([]), n, 3, 0)
        assert off.tolist() == [0] * (n + 1) and len(nbrs) == 0
    off, nbrs = capi.knn_hits(records(hits), 5, 0, 0)   # k = 0: nothing
    assert off.tolist() == [0] * 6 and len(nbrs) == 0
    L = capi.lib()
    L.rk_knn_hits.argtypes = HITS_ARGTYPES
    off = np.full(6, 77, dtype=np.uint64)
    out, n_out = C.c_void_p(5), C.c_uint64(7)
    assert L.rk_knn_hits(None, 0, 5, 3, 0, off.ctypes.data, C.byref(out), C.byref(n_out)) == 0   # a list of no hits may be NULL
    assert off.tolist() == [0] * 6 and n_out.value == 0 and out.value is None


# ---- rk_knn_merge ---------------------------------------------------------------------------------------------------------
def test_merge_of_parts_equals_the_whole():
    for hits, n, metric, rng in graphs(64, 300):
        rec = records(hits)
        for k in (1, 2, 3, n):
            whole = capi.knn_hits(rec, n, k, metric)
            compare(whole, hits, n, k, metric)
            parts = int(rng.integers(2, 4))
            owner = rng.integers(0, parts, size=len(rec))
            folded = (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=capi.HIT_DTYPE))
            for p in range(parts):
                one = capi.knn_hits(rec[owner == p], n, k, metric)
                folded = capi.knn_merge(folded[0], folded[1], one[0], one[1], n, k, metric)
            assert np.array_equal(folded[0], whole[0]) and np.array_equal(folded[1], whole[1])
            same = capi.knn_merge(whole[0], whole[1], whole[0], whole[1], n, k, metric)   # merge(a, a) == a: a pair in both counts once
            assert np.array_equal(same[0], whole[0]) and np.array_equal(same[1], whole[1])
            if len(rec):   # a pair given in both inputs appears once in each of its two lists
                shared = np.arange(len(rec)) == int(rng.integers(len(rec)))
                one = capi.knn_hits(rec[(owner == 0) | shared], n, k, metric)
                two = capi.knn_hits(rec[(owner != 0) | shared], n, k, metric)
                got = capi.knn_merge(one[0], one[1], two[0], two[1], n, k, metric)
                assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
            # inputs with longer lists than k are cut to k
            long_ = capi.knn_hits(rec, n, n, metric)
            empty = (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=capi.HIT_DTYPE))
            for a, b in ((long_, empty), (empty, long_), (long_, long_)):
                cut = capi.knn_merge(a[0], a[1], b[0], b[1], n, k, metric)
                assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1])


def test_merge_accepts_lists_in_any_order_and_may_write_over_its_offsets():
    hits = [(0, 1, 20, 50, 50), (0, 2, 40, 60, 60), (0, 3, 60, 70, 70), (1, 2, 25, 50, 50)]
    rec = records(hits)
    whole = capi.knn_hits(rec, 4, 2, 0)
    a = capi.knn_hits(rec, 4, 4, 0)
    backwards = np.concatenate([a[1][int(a[0][v]): int(a[0][v + 1])][::-1] for v in range(4)])
    empty = (np.zeros(5, dtype=np.uint64), np.zeros(0, dtype=capi.HIT_DTYPE))
    got = capi.knn_merge(a[0], backwards, empty[0], empty[1], 4, 2, 0)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    L = capi.lib()
    L.rk_knn_merge.argtypes = MERGE_ARGTYPES
    a_off = a[0].copy()
    out, n_out = C.c_void_p(), C.c_uint64()
    assert L.rk_knn_merge(a_off.ctypes.data, a[1].ctypes.data, empty[0].ctypes.data, None, 4, 2, 0, a_off.ctypes.data, C.byref(out), C.byref(n_out)) == 0
    assert a_off.tolist() == whole[0].tolist() and n_out.value == len(whole[1])
    L.rk_free_host(out)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_knn_hits_refusals():
    L = capi.lib()
    L.rk_knn_hits.argtypes = HITS_ARGTYPES
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)])
    off = np.full(5, 77, dtype=np.uint64)
    out, n_out = C.c_void_p(), C.c_uint64()
    for bad in ([(0, 4, 25, 50, 50)], [(4, 5, 25, 50, 50)], [(1, 0xFFFFFFFF, 25, 50, 50)], [(2, 2, 25, 50, 50)]):
        both = np.concatenate([good, records(bad)])
        assert L.rk_knn_hits(both.ctypes.data, 3, 4, 2, 0, off.ctypes.data, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
        with pytest.raises(capi.RkError) as e:
            capi.knn_hits(both, 4, 2, 0)
        assert e.value.code == RK_ERR_ARG
    assert L.rk_knn_hits(None, 2, 4, 2, 0, off.ctypes.data, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
    assert L.rk_knn_hits(good.ctypes.data, 2, 4, 2, 0, None, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
    assert L.rk_knn_hits(good.ctypes.data, 2, 4, 2, 0, off.ctypes.data, None, C.byref(n_out)) == RK_ERR_ARG
    assert L.rk_knn_hits(good.ctypes.data, 2, 4, 2, 0, off.ctypes.data, C.byref(out), None) == RK_ERR_ARG
    assert np.all(off == 77)   # refused before anything is written
    assert L.rk_knn_hits(good.ctypes.data, 2, 4, 2, 0, off.ctypes.data, C.byref(out), C.byref(n_out)) == 0
    assert off.tolist() == [0, 1, 2, 3, 4] and n_out.value == 4
    L.rk_free_host(out)


def test_knn_merge_refusals():
    L = capi.lib()
    L.rk_knn_merge.argtypes = MERGE_ARGTYPES
    hits = [(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)]
    a_off, a = capi.knn_hits(records(hits), 4, 2, 0)
    assert a_off.tolist() == [0, 1, 2, 3, 4]
    off = np.full(5, 77, dtype=np.uint64)
    out, n_out = C.c_void_p(), C.c_uint64()

    def call(b_off, b, n=4, a_off_=a_off, a_=a, off_=off, out_=True, n_out_=True):
        return L.rk_knn_merge(a_off_.ctypes.data if a_off_ is not None else None, a_.ctypes.data if a_ is not None else None,
                              b_off.ctypes.data if b_off is not None else None, b.ctypes.data if b is not None else None, n, 2, 0,
                              off_.ctypes.data if off_ is not None else None, C.byref(out) if out_ else None, C.byref(n_out) if n_out_ else None)
    one = np.array([0, 1, 1, 1, 1], dtype=np.uint64)
    for bad in ((0, 4, 25, 50, 50), (0, 0xFFFFFFFF, 25, 50, 50), (0, 0, 25, 50, 50)):   # a genome >= n, row == col
        assert call(one, records([bad])) == RK_ERR_ARG
    assert call(one, records([(1, 2, 25, 50, 50)])) == RK_ERR_ARG   # not incident to genome 0, whose list holds it
    assert call(np.array([0, 2, 1, 1, 1], dtype=np.uint64), records([(0, 1, 25, 50, 50), (0, 2, 25, 50, 50)])) == RK_ERR_ARG   # offsets that do not ascend
    assert call(one, None) == RK_ERR_ARG   # records missing
    assert call(None, a) == RK_ERR_ARG
    assert call(a_off, a, a_off_=None) == RK_ERR_ARG
    assert call(a_off, a, off_=None) == RK_ERR_ARG
    assert call(a_off, a, out_=False) == RK_ERR_ARG
    assert call(a_off, a, n_out_=False) == RK_ERR_ARG
    assert np.all(off == 77)   # refused before anything is written
    with pytest.raises(capi.RkError) as e:
        capi.knn_merge(a_off, a, one, records([(1, 2, 25, 50, 50)]), 4, 2, 0)
    assert e.value.code == RK_ERR_ARG
    assert call(one, records([(0, 2, 20, 50, 50)])) == 0
    assert off.tolist() == [0, 2, 3, 4, 5] and n_out.value == 5
    L.rk_free_host(out)
    zero = np.zeros(5, dtype=np.uint64)
    assert call(zero, None, a_off_=zero, a_=None) == 0 and n_out.value == 0 and out.value is None   # empty lists need no records


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_knn_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_knn_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p),
                              C.POINTER(C.c_uint64), C.POINTER(capi.KnnStats)]
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    off = np.zeros(5, dtype=np.uint64)
    nbrs, n, st = C.c_void_p(), C.c_uint64(), capi.KnnStats()
    assert L.rk_knn_rows(None, None, C.byref(opts), 3, off.ctypes.data, C.byref(nbrs), C.byref(n), C.byref(st)) == RK_ERR_ARG
    assert L.rk_knn_rows(None, None, None, 3, None, None, None, None) == RK_ERR_ARG


def test_knn_symbols_are_exported():
    L = capi.lib()
    for name in ("rk_knn_rows", "rk_knn_hits", "rk_knn_merge"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.knn_rows) and callable(capi.knn_hits) and callable(capi.knn_merge)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_KNN_SELECT 8\b", hdr)


def test_knn_stats_has_the_headers_size():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    m = re.search(r"typedef struct rk_knn_stats \{(.*?)\} rk_knn_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    width = {"uint64_t": 8, "uint32_t": 4}
    fields = [(t, name) for t, name in re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [name for _, name in fields] == [name for name, _ in capi.KnnStats._fields_]
    assert [name for _, name in fields] == ["edges", "borderline", "borderline_kept", "neighbours", "join_attempts", "border_attempts", "max_degree", "path"]
    assert C.sizeof(capi.KnnStats) == sum(width[t] for t, _ in fields) == 48
    for (t, name), (_, ctype) in zip(fields, capi.KnnStats._fields_):
        assert C.sizeof(ctype) == width[t], name
