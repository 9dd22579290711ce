"""The host side of the forest (rk_forest_merge, rk_forest_cut), the refusals of rk_forest_rows that need no context and the
size of rk_forest_stats -- against tests/_forest_ref.py, a Kruskal with exact rational weights that is itself checked against
brute force over every spanning forest of small graphs."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _forest_ref as fr
from rabbitkssd_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG = -1
KMER = 20
# (common, size0, size1): few distinct ratios, several of them from different counts -- 25/75 = 20/60 = 30/90 (metric 0),
# 25/50 = 20/40 = 30/60 = 26/52 (metric 1), 40/50 both ways
TRIPLES = [(25, 50, 50), (20, 40, 40), (30, 60, 60), (26, 50, 51), (26, 52, 60), (40, 45, 45), (40, 50, 80), (36, 40, 50), (10, 20, 20),
           (45, 50, 50), (50, 50, 50)]


def records(hits, metric):
    """hits as rk_hit records with the reference's jorc and dist"""
    rec = np.zeros(len(hits), dtype=capi.HIT_DTYPE)
    for k, h in enumerate(hits):
        rec[k] = (h[0], h[1], h[2], h[3], h[4], 0) + fr.distance(h, metric, KMER)
    return rec


def random_hits(rng, n, m, seen=None):
    """m hits over n genomes; a pair has ONE record (as in a join's hit list): drawn again, here or in another list that shares
    `seen`, it comes with the same counts"""
    seen = {} if seen is None else seen
    hits = []
    for _ in range(m if n > 1 else 0):
        pair = tuple(sorted(rng.choice(n, size=2, replace=False).tolist()))
        if pair not in seen:
            seen[pair] = TRIPLES[int(rng.integers(len(TRIPLES)))]
        hits.append(pair + seen[pair])
    return hits


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_kruskal_against_brute_force():
    rng = np.random.default_rng(40)
    for case in range(60):
        n = int(rng.integers(2, 13))
        metric = case % 2
        pairs = list(itertools.combinations(range(n), 2))
        m = int(rng.integers(0, min(len(pairs), 11) + 1))
        hits = [pairs[i] + TRIPLES[int(rng.integers(len(TRIPLES)))] for i in rng.choice(len(pairs), size=m, replace=False)]
        forest = fr.kruskal(hits, n, metric)
        whole = fr.components([(h[0], h[1]) for h in hits], n)
        assert fr.components([(h[0], h[1]) for h in forest], n) == whole
        size = n - len(set(whole))
        assert len(forest) == size
        best_sum, best_keys = None, None
        for sub in itertools.combinations(hits, size):   # every spanning forest: `size` edges that connect what the graph connects
            if fr.components([(h[0], h[1]) for h in sub], n) != whole:
                continue
            total = sum(-fr.ratio(h, metric) for h in sub)
            keys = sorted(fr.edge_key(h, metric) for h in sub)
            best_sum = total if best_sum is None else min(best_sum, total)
            best_keys = keys if best_keys is None else min(best_keys, keys)
        assert sum(-fr.ratio(h, metric) for h in forest) == best_sum, case
        assert [fr.edge_key(h, metric) for h in forest] == best_keys, case   # in order, and the one forest the strict order singles out
        for t in sorted({fr.ratio(h, metric) for h in hits}):   # cut anywhere: the components of the edges above t
            assert (fr.components([(h[0], h[1]) for h in forest if fr.ratio(h, metric) > t], n)
                    == fr.components([(h[0], h[1]) for h in hits if fr.ratio(h, metric) > t], n)), (case, t)


# ---- rk_forest_merge ----------------------------------------------------------------------------------------------------
def test_merge_equals_the_reference_kruskal():
    rng = np.random.default_rng(41)
    for case in range(200):
        n = 1 + case * 499 // 199   # 1 .. 500
        metric = case % 2
        seen = {}
        a = random_hits(rng, n, int(rng.integers(0, 2 * n)), seen)
        b = random_hits(rng, n, int(rng.integers(0, 2 * n)), seen)
        if case % 3 == 0:   # forests as inputs, as the folds of shards have them
            a, b = fr.kruskal(a, n, metric), fr.kruskal(b, n, metric)
        want = fr.kruskal(a + b, n, metric)
        ra, rb = records(a, metric), records(b, metric)
        got = capi.forest_merge(ra, rb, n, metric)
        assert fr.hit_tuples(got) == want, (case, n)
        wrec = records(want, metric)
        assert np.array_equal(got["dist"], wrec["dist"]) and np.array_equal(got["jorc"], wrec["jorc"])   # records travel unchanged
        assert fr.hit_tuples(capi.forest_merge(rb, ra, n, metric)) == want, (case, n)
    assert n == 500


def test_merge_ties_empty_lists_and_forests_of_one_list():
    # 25/75 and 20/60 tie under metric 0: (row, col) decides; 26/75 is nearer than both
    tri = [(1, 2, 25, 50, 50), (0, 2, 20, 40, 40), (0, 1, 26, 50, 51)]
    got = capi.forest_merge(records(tri[:1], 0), records(tri[1:], 0), 3, 0)
    assert fr.hit_tuples(got) == [tri[2], tri[1]] == fr.kruskal(tri, 3, 0)
    empty = records([], 0)
    assert len(capi.forest_merge(empty, empty, 5, 0)) == 0
    assert len(capi.forest_merge(empty, empty, 0, 1)) == 0
    rng = np.random.default_rng(42)
    for metric in (0, 1):
        hits = random_hits(rng, 40, 200)
        want = fr.kruskal(hits, 40, metric)
        assert fr.hit_tuples(capi.forest_merge(records(hits, metric), empty, 40, metric)) == want
        assert fr.hit_tuples(capi.forest_merge(empty, records(hits, metric), 40, metric)) == want
        f = records(want, metric)
        assert fr.hit_tuples(capi.forest_merge(f, f, 40, metric)) == want   # idempotent
    L = capi.lib()
    L.rk_forest_merge.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    out, n_out = C.c_void_p(), C.c_uint64(7)
    assert L.rk_forest_merge(None, 0, None, 0, 9, 0, C.byref(out), C.byref(n_out)) == 0 and n_out.value == 0   # a list of no edges may be NULL
    L.rk_free_host(out)


def test_merge_refuses_genomes_beyond_n_and_null_pointers():
    L = capi.lib()
    L.rk_forest_merge.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)], 0)
    out, n_out = C.c_void_p(), C.c_uint64()
    for bad in ([(0, 4, 25, 50, 50)], [(4, 5, 25, 50, 50)], [(1, 0xFFFFFFFF, 25, 50, 50)]):
        bad = records(bad, 0)
        assert L.rk_forest_merge(bad.ctypes.data, 1, good.ctypes.data, 2, 4, 0, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
        assert L.rk_forest_merge(good.ctypes.data, 2, bad.ctypes.data, 1, 4, 0, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
        with pytest.raises(capi.RkError) as e:
            capi.forest_merge(good, bad, 4, 0)
        assert e.value.code == RK_ERR_ARG
    assert L.rk_forest_merge(None, 2, good.ctypes.data, 2, 4, 0, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
    assert L.rk_forest_merge(good.ctypes.data, 2, None, 2, 4, 0, C.byref(out), C.byref(n_out)) == RK_ERR_ARG
    assert L.rk_forest_merge(good.ctypes.data, 2, good.ctypes.data, 2, 4, 0, None, C.byref(n_out)) == RK_ERR_ARG
    assert L.rk_forest_merge(good.ctypes.data, 2, good.ctypes.data, 2, 4, 0, C.byref(out), None) == RK_ERR_ARG


# ---- rk_forest_cut ------------------------------------------------------------------------------------------------------
def test_cut_equals_a_union_find():
    rng = np.random.default_rng(43)
    for case in range(100):
        n = 1 + case * 5
        metric = case % 2
        hits = random_hits(rng, n, int(rng.integers(0, 2 * n)))
        rec = records(hits, metric)   # any edge list, a forest or not
        for t in [0.0, 1.0] + sorted(set(rec["dist"].tolist())) + [float(np.nextafter(d, 1.0)) for d in set(rec["dist"].tolist())]:
            want = fr.components([(h[0], h[1]) for h, d in zip(hits, rec["dist"].tolist()) if d < t], n)   # strict <
            got = capi.forest_cut(rec, n, t)
            assert got.dtype == np.uint32 and got.tolist() == want, (case, t)
        forest = records(fr.kruskal(hits, n, metric), metric)   # the cut of the forest is the cut of the graph
        for t in sorted(set(rec["dist"].tolist())):
            assert np.array_equal(capi.forest_cut(forest, n, t), capi.forest_cut(rec, n, t))
    assert len(capi.forest_cut(records([], 0), 0, 0.5)) == 0


def test_cut_refuses_genomes_beyond_n_and_null_pointers():
    L = capi.lib()
    L.rk_forest_cut.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p]
    good = records([(0, 1, 25, 50, 50)], 0)
    labels = np.full(4, 77, dtype=np.uint32)
    for bad in ([(0, 4, 25, 50, 50)], [(7, 9, 25, 50, 50)]):
        bad = records(bad, 0)
        assert L.rk_forest_cut(bad.ctypes.data, 1, 4, 0.5, labels.ctypes.data) == RK_ERR_ARG
        assert np.all(labels == 77)   # refused before anything is written
        with pytest.raises(capi.RkError) as e:
            capi.forest_cut(bad, 4, 0.5)
        assert e.value.code == RK_ERR_ARG
    assert L.rk_forest_cut(None, 1, 4, 0.5, labels.ctypes.data) == RK_ERR_ARG
    assert L.rk_forest_cut(good.ctypes.data, 1, 4, 0.5, None) == RK_ERR_ARG
    assert L.rk_forest_cut(good.ctypes.data, 1, 4, 0.5, labels.ctypes.data) == 0 and labels.tolist() == [0, 0, 2, 3]


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_forest_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_forest_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                 C.POINTER(capi.ForestStats)]
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    edges, n, st = C.c_void_p(), C.c_uint64(), capi.ForestStats()
    assert L.rk_forest_rows(None, None, C.byref(opts), C.byref(edges), C.byref(n), C.byref(st)) == RK_ERR_ARG
    assert L.rk_forest_rows(None, None, None, None, None, None) == RK_ERR_ARG


def test_forest_symbols_are_exported():
    L = capi.lib()
    for name in ("rk_forest_rows", "rk_forest_merge", "rk_forest_cut"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.forest_rows) and callable(capi.forest_merge) and callable(capi.forest_cut)


def test_forest_stats_has_the_headers_size():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    m = re.search(r"typedef struct rk_forest_stats \{(.*?)\} rk_forest_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    width = {"uint64_t": 8, "uint32_t": 4}
    fields = [(t, name) for t, name in re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [name for _, name in fields] == [name for name, _ in capi.ForestStats._fields_]
    assert [name for _, name in fields] == ["edges", "borderline", "borderline_kept", "join_attempts", "border_attempts", "rounds", "n_trees"]
    assert C.sizeof(capi.ForestStats) == sum(width[t] for t, _ in fields) == 40
    for (t, name), (_, ctype) in zip(fields, capi.ForestStats._fields_):
        assert C.sizeof(ctype) == width[t], name
