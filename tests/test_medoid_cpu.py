"""The host side of the medoids and census of a clustering (rk_medoid_hits, rk_medoid_merge, rk_medoid_pick), the refusals of
rk_medoid_rows that need no context and the sizes of its structures -- against tests/_medoid_ref.py: the rule with Python integers and
exact rational ratios, itself checked against the properties that single its result out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _medoid_ref as mr
from rabbitkssd_amd import capi
from test_greedy_cpu import TRIPLES, random_graph, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
NONE = mr.NONE
HITS_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(capi.MedoidGenomes)]
MERGE_ARGTYPES = [C.POINTER(capi.MedoidGenomes), C.POINTER(capi.MedoidGenomes), C.c_uint32, C.c_int, C.POINTER(capi.MedoidGenomes)]
PICK_ARGTYPES = [C.c_void_p, C.POINTER(capi.MedoidGenomes), C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]


def random_labels(rng, n):
    """labels of every form: below n without being a member of the cluster, NONE, few clusters or many"""
    kinds = int(rng.integers(1, n + 1))
    names = rng.choice(n, size=kinds, replace=False)
    labels = [int(names[int(rng.integers(kinds))]) for _ in range(n)]
    for v in range(n):
        if rng.integers(5) == 0:
            labels[v] = NONE
    return labels


def cases(seed, count):
    """(hits, n, labels, metric, rng) of `count` random graphs over TRIPLES (20/60 ties 25/75 under both metrics), n <= 14"""
    rng = np.random.default_rng(seed)
    for case in range(count):
        n = int(rng.integers(1, 15))
        yield random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))]), n, random_labels(rng, n), case % 2, rng


def as_ref(got):
    """(in_deg, out_deg, central, far_in, near_out) of the library in the reference's form"""
    def hits_or_none(rec):
        absent = rec["row"] == NONE
        assert np.all(rec["col"][absent] == NONE) and all(not rec[f][absent].any() for f in ("common", "size0", "size1", "pad", "jorc", "dist"))
        return [None if a else t for a, t in zip(absent.tolist(), mr.hit_tuples(rec))]
    return [got[0].tolist(), got[1].tolist(), got[2].tolist(), hits_or_none(got[3]), hits_or_none(got[4])]


def clusters_as_ref(picked):
    def hit(rec):
        return None if rec["row"] == NONE else tuple(int(rec[f]) for f in ("row", "col", "common", "size0", "size1"))
    return [{"label": int(c["label"]), "size": int(c["size"]), "medoid": int(c["medoid"]), "in_edges": int(c["in_edges"]), "central": int(c["central"]),
             "weakest_in": hit(c["weakest_in"]), "nearest_out": hit(c["nearest_out"])} for c in picked]


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_has_the_characterising_properties_on_small_graphs():
    """Every graph and every assignment of labels up to 3 vertices, every 7th case of 4 vertices and every 4001st of 5 (all of them:
    python tests/_medoid_ref.py, a quarter of an hour)"""
    assert mr.TRIPLES == TRIPLES
    ties = moved = 0
    for n, stride in ((1, 1), (2, 1), (3, 1), (4, 7), (5, 4001)):
        total = (1 << (n * (n - 1) // 2)) * (n + 1) ** n
        count, t, m = mr.exhaustive(n, stride, first=n % stride)
        assert count == -(-(total - n % stride) // stride)
        ties += t
        moved += m
    assert ties > 2000 and moved > 300


def test_checker_refuses_what_is_not_the_rule():
    # a triangle 0 1 2 in cluster 2, genome 3 in cluster 0 hangs on 1 and on 2, genome 4 unlabelled hangs on 0: 25/75 ties 20/60
    hits = [(0, 1, 25, 50, 50), (0, 2, 20, 40, 40), (1, 2, 40, 60, 60), (1, 3, 20, 40, 40), (2, 3, 25, 50, 50), (0, 4, 60, 70, 70)]
    labels = [2, 2, 2, 0, NONE]
    g = mr.genomes(hits, 5, labels, 0)
    clusters = mr.pick(labels, g, 0)
    assert g[0] == [2, 2, 2, 0, 0] and g[1] == [1, 1, 1, 2, 1]
    assert g[3][:3] == [hits[0], hits[0], hits[1]] and g[4] == [hits[5], hits[3], hits[4], hits[3], hits[5]]   # ties: the smaller neighbour
    assert g[2][1] == (25 << 32) // 75 + (40 << 32) // 80 and [c["medoid"] for c in clusters] == [3, 1]
    assert clusters[1]["weakest_in"] == hits[0] and clusters[1]["nearest_out"] == hits[5] and clusters[0]["nearest_out"] == hits[3]
    mr.check_properties(hits, 5, labels, 0, g, clusters)
    for at, v, wrong in ((0, 0, 1), (1, 3, 1), (2, 1, g[2][1] + 1), (3, 0, hits[1]), (3, 3, hits[3]), (4, 1, hits[0]), (4, 3, hits[4]), (4, 4, None)):
        bad = [list(x) for x in g]
        bad[at][v] = wrong
        with pytest.raises(AssertionError):
            mr.check_properties(hits, 5, labels, 0, bad, clusters)
    for key, wrong in (("medoid", 0), ("size", 2), ("in_edges", 2), ("weakest_in", hits[1]), ("weakest_in", None), ("nearest_out", hits[3]), ("central", 1)):
        bad = [dict(c) for c in clusters]
        bad[1][key] = wrong
        with pytest.raises(AssertionError):
            mr.check_properties(hits, 5, labels, 0, g, bad)
    with pytest.raises(AssertionError):
        mr.check_properties(hits, 5, labels, 0, g, clusters[:1])


# ---- rk_medoid_hits and rk_medoid_pick ------------------------------------------------------------------------------------
def test_medoid_hits_and_pick_equal_the_reference_on_random_graphs():
    ties = moved = strangers = 0
    for hits, n, labels, metric, rng in cases(90, 300):
        rec = records(hits)
        got = capi.medoid_hits(rec, n, labels, metric)
        assert [a.dtype for a in got] == [np.uint32, np.uint32, np.uint64, capi.HIT_DTYPE, capi.HIT_DTYPE]
        want = mr.genomes(hits, n, labels, metric)
        assert as_ref(got) == list(want)
        by_pair = {(int(r["row"]), int(r["col"])): r for r in rec}
        for arr in got[3:]:   # the caller's records, unchanged: the marks in jorc and dist travel
            for r in arr[arr["row"] != NONE]:
                assert r == by_pair[(int(r["row"]), int(r["col"]))]
        picked = capi.medoid_pick(labels, got, metric)
        assert picked.dtype == capi.MEDOID_CLUSTER_DTYPE and not picked["pad"].any()
        clusters = clusters_as_ref(picked)
        assert clusters == mr.pick(labels, want, metric)
        mr.check_properties(hits, n, labels, metric, as_ref(got), clusters)
        bare = capi.medoid_hits(rec, n, labels, metric, records=False)   # no record arrays: the same sums, no cluster records
        assert bare[3] is None and bare[4] is None and same(bare[:3], got[:3])
        for g in (bare, got[:3] + (got[3], None), got[:3] + (None, got[4])):
            lone = capi.medoid_pick(labels, g, metric)
            assert np.all(lone["weakest_in"]["row"] == NONE) and np.all(lone["nearest_out"]["col"] == NONE)
            assert all(np.array_equal(lone[f], picked[f]) for f in ("label", "size", "medoid", "in_edges", "central"))
        shuffled = rec[rng.permutation(len(rec))]   # the order of the hits does not matter
        swapped = shuffled.copy()                   # nor which endpoint is the row: the record comes back row first, its sizes with it
        swapped["row"], swapped["col"], swapped["size0"], swapped["size1"] = shuffled["col"], shuffled["row"], shuffled["size1"], shuffled["size0"]
        for again in (capi.medoid_hits(shuffled, n, labels, metric), capi.medoid_hits(swapped, n, labels, metric)):
            assert same(again, got)
        for v in range(n):
            for best, group in ((want[3][v], True), (want[4][v], False)):
                if best is not None:
                    ties += sum(v in h[:2] and mr.inside(h, labels) == group and mr.cross(h, best, metric) == 0 for h in hits) > 1
        moved += sum(c["medoid"] != min(v for v in range(n) if labels[v] == c["label"]) for c in clusters)
        strangers += sum(labels[c["label"]] != c["label"] for c in clusters)
    assert ties > 300 and moved > 100 and strangers > 100   # equal ratios decided, central members, labels that are no members


def split(rec, rng, parts):
    where = rng.integers(parts, size=len(rec))
    return [rec[where == p] for p in range(parts)]


def test_medoid_merge_of_random_splits_equals_the_whole():
    for hits, n, labels, metric, rng in cases(91, 150):
        rec = records(hits)
        whole = capi.medoid_hits(rec, n, labels, metric)
        two = [capi.medoid_hits(part, n, labels, metric) for part in split(rec, rng, 2)]
        assert same(capi.medoid_merge(two[0], two[1], n, metric), whole)
        assert same(capi.medoid_merge(two[1], two[0], n, metric), whole)
        a, b, c = [capi.medoid_hits(part, n, labels, metric) for part in split(rec, rng, 3)]
        left = capi.medoid_merge(capi.medoid_merge(a, b, n, metric), c, n, metric)
        right = capi.medoid_merge(a, capi.medoid_merge(b, c, n, metric), n, metric)
        assert same(left, whole) and same(right, whole)   # associative
        assert as_ref(left) == list(mr.merge(mr.merge(as_ref(a), as_ref(b), metric), as_ref(c), metric))
        # one side without a record array: the result has none of that kind; the other kind and the sums as before
        lone = capi.medoid_merge(a[:3] + (None, a[4]), b, n, metric)
        ab = capi.medoid_merge(a, b, n, metric)
        assert lone[3] is None and same(lone[:3] + lone[4:], ab[:3] + ab[4:])
        # out may alias a
        L = capi.lib()
        L.rk_medoid_merge.argtypes = MERGE_ARGTYPES
        mine = tuple(x.copy() for x in a)
        ga, gb = capi._medoid_struct(mine), capi._medoid_struct(b)
        assert L.rk_medoid_merge(C.byref(ga), C.byref(gb), n, metric, C.byref(ga)) == 0
        assert same(mine, ab)


def test_labels_that_are_not_members_of_their_cluster():
    hits = [(0, 1, 60, 70, 70), (1, 2, 40, 60, 60), (0, 2, 20, 50, 50), (2, 3, 25, 50, 50)]
    labels = [3, 3, 3, 0]   # the cluster of 0, 1 and 2 is called 3, the singleton 3 is called 0
    got = capi.medoid_hits(records(hits), 4, labels, 0)
    assert got[0].tolist() == [2, 2, 2, 0] and got[1].tolist() == [0, 0, 1, 1]
    picked = capi.medoid_pick(labels, got, 0)
    assert picked["label"].tolist() == [0, 3] and picked["size"].tolist() == [1, 3] and picked["medoid"].tolist() == [3, 1]
    assert picked["in_edges"].tolist() == [0, 3] and int(picked["central"][1]) == (60 << 32) // 80 + (40 << 32) // 80
    assert clusters_as_ref(picked) == mr.pick(labels, mr.genomes(hits, 4, labels, 0), 0)
    assert picked["weakest_in"][0]["row"] == NONE and clusters_as_ref(picked)[0]["nearest_out"] == hits[3]
    for n in (0, 1, 5):   # no hits at all; all unlabelled: no cluster
        got = capi.medoid_hits(records([]), n, list(range(n)), 0)
        assert not got[0].any() and not got[1].any() and not got[2].any() and np.all(got[3]["row"] == NONE) and np.all(got[4]["col"] == NONE)
        picked = capi.medoid_pick(list(range(n)), got, 0)
        assert picked["medoid"].tolist() == list(range(n)) and picked["size"].tolist() == [1] * n
        assert len(capi.medoid_pick([NONE] * n, got, 0)) == 0
    one_q = capi.medoid_hits(records([(0, 1, 70, 70, 70)]), 2, [0, 0], 1)   # common == u: q = 2^32 exactly
    assert one_q[2].tolist() == [1 << 32, 1 << 32]


# ---- refusals: nothing is written -----------------------------------------------------------------------------------------
def marked(n):
    arrays = (np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint64), np.zeros(n, dtype=capi.HIT_DTYPE),
              np.zeros(n, dtype=capi.HIT_DTYPE))
    for rec in arrays[3:]:
        rec["row"] = rec["col"] = rec["common"] = 77
    return arrays


def untouched(arrays):
    return all(np.all(a == 77) for a in arrays[:3]) and all(np.all(r["row"] == 77) and np.all(r["common"] == 77) for r in arrays[3:])


def test_medoid_hits_refusals_write_nothing():
    L = capi.lib()
    L.rk_medoid_hits.argtypes = HITS_ARGTYPES
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)])
    labels = np.array([0, 0, 2, NONE], dtype=np.uint32)
    out = marked(4)
    g = capi._medoid_struct(out)
    for bad in ([(0, 4, 25, 50, 50)], [(4, 5, 25, 50, 50)], [(1, 0xFFFFFFFF, 25, 50, 50)], [(2, 2, 25, 50, 50)]):
        both = np.concatenate([good, records(bad)])
        assert L.rk_medoid_hits(both.ctypes.data, 3, 4, labels.ctypes.data, 0, C.byref(g)) == RK_ERR_ARG
        with pytest.raises(capi.RkError) as e:
            capi.medoid_hits(both, 4, labels, 0)
        assert e.value.code == RK_ERR_ARG
    for bad in ([(1, 2, 0, 50, 50)], [(1, 2, 60, 50, 50)], [(1, 2, -1, 50, 50)]):   # outside 0 < common <= u: q is not defined
        both = np.concatenate([good, records(bad)])
        assert L.rk_medoid_hits(both.ctypes.data, 3, 4, labels.ctypes.data, 1, C.byref(g)) == RK_ERR_UNSUPPORTED
    for wrong in (4, 5, 0xFFFFFFFE):   # a label that is neither below n nor NONE
        lab = labels.copy()
        lab[1] = wrong
        assert L.rk_medoid_hits(good.ctypes.data, 2, 4, lab.ctypes.data, 0, C.byref(g)) == RK_ERR_ARG
    assert L.rk_medoid_hits(None, 2, 4, labels.ctypes.data, 0, C.byref(g)) == RK_ERR_ARG
    assert L.rk_medoid_hits(good.ctypes.data, 2, 4, None, 0, C.byref(g)) == RK_ERR_ARG
    assert L.rk_medoid_hits(good.ctypes.data, 2, 4, labels.ctypes.data, 0, None) == RK_ERR_ARG
    for k in range(3):   # the three sums are required
        part = list(out)
        part[k] = None
        lone = capi._medoid_struct(part)
        assert L.rk_medoid_hits(good.ctypes.data, 2, 4, labels.ctypes.data, 0, C.byref(lone)) == RK_ERR_ARG
    assert untouched(out)   # refused before anything is written
    assert L.rk_medoid_hits(good.ctypes.data, 2, 4, labels.ctypes.data, 0, C.byref(g)) == 0
    assert out[0].tolist() == [1, 1, 0, 0] and out[1].tolist() == [0, 0, 1, 1] and out[4]["row"].tolist() == [NONE, NONE, 2, 2]
    empty = capi.MedoidGenomes()
    assert L.rk_medoid_hits(None, 0, 0, None, 0, C.byref(empty)) == 0   # no genome: nothing to write


def test_medoid_merge_and_pick_refusals_write_nothing():
    L = capi.lib()
    L.rk_medoid_merge.argtypes = MERGE_ARGTYPES
    L.rk_medoid_pick.argtypes = PICK_ARGTYPES
    hits = records([(0, 1, 25, 50, 50), (1, 2, 20, 40, 40), (2, 3, 60, 70, 70)])
    labels = np.array([0, 0, 2, NONE], dtype=np.uint32)
    a = capi.medoid_hits(hits[:2], 4, labels, 0)
    b = capi.medoid_hits(hits[2:], 4, labels, 0)
    out = marked(4)
    ga, gb, go = capi._medoid_struct(a), capi._medoid_struct(b), capi._medoid_struct(out)
    assert L.rk_medoid_merge(None, C.byref(gb), 4, 0, C.byref(go)) == RK_ERR_ARG
    assert L.rk_medoid_merge(C.byref(ga), None, 4, 0, C.byref(go)) == RK_ERR_ARG
    assert L.rk_medoid_merge(C.byref(ga), C.byref(gb), 4, 0, None) == RK_ERR_ARG
    for k in range(3):
        part = list(a)
        part[k] = None
        lone = capi._medoid_struct(part)
        assert L.rk_medoid_merge(C.byref(lone), C.byref(gb), 4, 0, C.byref(go)) == RK_ERR_ARG
    for field, v, value in (("col", 1, 4), ("row", 1, 2), ("col", 0, 3), ("row", 2, 3)):   # beyond n; row >= col; not a pair of the genome (twice)
        rec = tuple(x.copy() for x in a)
        rec[4][field][v] = value
        gr = capi._medoid_struct(rec)
        assert L.rk_medoid_merge(C.byref(gr), C.byref(gb), 4, 0, C.byref(go)) == RK_ERR_ARG
        assert L.rk_medoid_merge(C.byref(gb), C.byref(gr), 4, 0, C.byref(go)) == RK_ERR_ARG
    assert untouched(out)
    assert L.rk_medoid_merge(C.byref(ga), C.byref(gb), 4, 0, C.byref(go)) == 0
    assert same(out, capi.medoid_hits(hits, 4, labels, 0))
    # rk_medoid_pick
    ptr, count = C.c_void_p(77), C.c_uint32(77)
    for lab in (None, np.array([0, 0, 2, 4], dtype=np.uint32)):
        assert L.rk_medoid_pick(lab.ctypes.data if lab is not None else None, C.byref(go), 4, 0, C.byref(ptr), C.byref(count)) == RK_ERR_ARG
    assert L.rk_medoid_pick(labels.ctypes.data, None, 4, 0, C.byref(ptr), C.byref(count)) == RK_ERR_ARG
    assert L.rk_medoid_pick(labels.ctypes.data, C.byref(go), 4, 0, None, C.byref(count)) == RK_ERR_ARG
    assert L.rk_medoid_pick(labels.ctypes.data, C.byref(go), 4, 0, C.byref(ptr), None) == RK_ERR_ARG
    assert ptr.value == 77 and count.value == 77
    with pytest.raises(capi.RkError) as e:
        capi.medoid_pick([0, 0, 2, 4], out, 0)
    assert e.value.code == RK_ERR_ARG
    assert L.rk_medoid_pick(None, C.byref(capi.MedoidGenomes()), 0, 0, C.byref(ptr), C.byref(count)) == 0 and count.value == 0 and not ptr.value


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_medoid_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_medoid_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.POINTER(capi.MedoidGenomes), C.POINTER(capi.MedoidStats)]
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    out = marked(4)
    g, st = capi._medoid_struct(out), capi.MedoidStats()
    labels = np.zeros(4, dtype=np.uint32)
    assert L.rk_medoid_rows(None, None, C.byref(opts), labels.ctypes.data, C.byref(g), C.byref(st)) == RK_ERR_ARG
    assert L.rk_medoid_rows(None, None, None, None, None, None) == RK_ERR_ARG
    assert untouched(out)


def test_medoid_symbols_are_exported():
    L = capi.lib()
    for name in ("rk_medoid_rows", "rk_medoid_hits", "rk_medoid_merge", "rk_medoid_pick"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.medoid_rows) and callable(capi.medoid_hits) and callable(capi.medoid_merge) and callable(capi.medoid_pick)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_MEDOID 11\b", hdr)
    assert re.search(r"#define RK_MEDOID_NONE 0xFFFFFFFFu\b", hdr) and capi.MEDOID_NONE == mr.NONE == capi.DBSCAN_NOISE == 0xFFFFFFFF


def test_medoid_structures_have_the_headers_sizes():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    width = {"uint64_t": 8, "uint32_t": 4, "rk_hit": capi.HIT_DTYPE.itemsize}

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for t, names in re.findall(r"\b(uint64_t|uint32_t|rk_hit)\s+([\w\s,*]+);", body):
            out += [(t, x.strip().lstrip("*")) for x in names.split(",")]
        return out
    st = fields("rk_medoid_stats")
    assert [x for _, x in st] == [x for x, _ in capi.MedoidStats._fields_] == ["edges", "borderline", "borderline_kept", "inside", "leaving", "join_attempts",
                                                                              "border_attempts"]
    assert C.sizeof(capi.MedoidStats) == sum(width[t] for t, _ in st) == 48
    cl = fields("rk_medoid_cluster")
    assert [x for _, x in cl] == ["label", "size", "medoid", "pad_", "in_edges", "central", "weakest_in", "nearest_out"]
    assert [x.rstrip("_") for _, x in cl] == list(capi.MEDOID_CLUSTER_DTYPE.names) and capi.MEDOID_CLUSTER_DTYPE.itemsize == sum(width[t] for t, _ in cl) == 112
    assert [capi.MEDOID_CLUSTER_DTYPE.fields[x][1] for x in capi.MEDOID_CLUSTER_DTYPE.names] == [0, 4, 8, 12, 16, 24, 32, 72]
    ge = fields("rk_medoid_genomes")
    assert [x for _, x in ge] == [x for x, _ in capi.MedoidGenomes._fields_] == ["in_deg", "out_deg", "central", "far_in", "near_out"]
    assert C.sizeof(capi.MedoidGenomes) == 40
