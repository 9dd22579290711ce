"""The host side of the placement of query genomes (rk_assign_hits), the refusals of rk_assign_rows that need no context and the sizes of
its structures -- against tests/_assign_ref.py: the rule with Python integers and exact rational ratios, itself checked against the
properties that single its result out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _assign_ref as ar
from rabbitkssd_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
NONE = ar.NONE
# 20/60 ties 25/75 under metric 0, 20/40 ties 25/50 under metric 1: equal ratios from different counts
TRIPLES = [(20, 50, 50), (40, 60, 60), (60, 70, 70), (20, 40, 40), (25, 50, 50)]
HITS_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(capi.AssignQueries)]
ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.POINTER(capi.AssignQueries), C.POINTER(capi.AssignStats)]


def records(hits):
    rec = np.zeros(len(hits), dtype=capi.HIT_DTYPE)
    for k, h in enumerate(hits):
        rec[k] = (h[0], h[1], h[2], h[3], h[4], 0, 0.25 + k, 0.5 + k)   # (jorc and dist: marks that must travel unchanged)
    return rec


def random_hits(rng, n_query, n_ref):
    """a random subset of the cells of n_query x n_ref, one record per cell, weights from TRIPLES"""
    cells = n_query * n_ref
    m = int(rng.integers(0, cells + 1))
    return [(int(c) // n_ref, int(c) % n_ref) + TRIPLES[int(rng.integers(len(TRIPLES)))] for c in rng.choice(cells, size=m, replace=False)] if m else []


def random_labels(rng, n):
    """labels of every form: below n without being a member of the cluster, NONE, few clusters or many"""
    kinds = int(rng.integers(1, n + 1))
    names = rng.choice(n, size=kinds, replace=False)
    return [NONE if rng.integers(4) == 0 else int(names[int(rng.integers(kinds))]) for _ in range(n)]


def as_ref(got):
    """(label, n_within, n_labelled, n_same, nearest, runner_up) of the library in the reference's form"""
    def hits_or_none(rec):
        absent = rec["row"] == NONE
        assert np.all(rec["col"][absent] == NONE) and all(not rec[f][absent].any() for f in ("common", "size0", "size1", "pad", "jorc", "dist"))
        return ar.record_tuples(rec)
    return [a.tolist() for a in got[:4]] + [hits_or_none(got[4]), hits_or_none(got[5])]


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def marked(q):
    out = tuple(np.full(q, 0xABABABAB, dtype=np.uint32) for _ in range(4)) + (np.zeros(q, dtype=capi.HIT_DTYPE), np.zeros(q, dtype=capi.HIT_DTYPE))
    out[4]["common"] = out[5]["common"] = 77
    return out


def untouched(out):
    return all(np.all(a == 0xABABABAB) for a in out[:4]) and all(np.all(a["common"] == 77) and not a["row"].any() for a in out[4:])


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_has_the_characterising_properties_on_small_patterns():
    """Every hit pattern and every labelling over {0, 1, NONE} of 1 and 2 queries x up to 3 references, every 5th case of 2 x 4 (all of
    them: python tests/_assign_ref.py)"""
    ties = seconds = unanchored = 0
    for n_q, n_r, stride in ((1, 1, 1), (1, 2, 1), (1, 3, 1), (1, 4, 1), (2, 1, 1), (2, 2, 1), (2, 3, 1), (2, 4, 5)):
        total = (1 << (n_q * n_r)) * (2 if n_r == 1 else 3) ** n_r
        count, t, s, u = ar.exhaustive(n_q, n_r, stride, first=1 % stride)
        assert count == -(-(total - 1 % stride) // stride)
        ties += t
        seconds += s
        unanchored += u
    assert ties > 300 and seconds > 1000 and unanchored > 300


def test_checker_refuses_what_is_not_the_rule():
    # query 0: references 0 (cluster 3) and 2 (cluster 1) tie at 25/75 = 20/60, reference 1 is nearer but unlabelled, reference 3 (cluster
    # 3) is farther; query 1 sees the unlabelled reference alone; query 2 sees nothing
    hits = [(0, 2, 20, 40, 40), (0, 0, 25, 50, 50), (0, 1, 60, 70, 70), (0, 3, 20, 50, 50), (1, 1, 40, 60, 60)]
    labels = [3, NONE, 1, 3]
    want = ar.assign(hits, 3, 4, labels, 0)
    assert want == ([3, NONE, NONE], [4, 1, 0], [3, 0, 0], [2, 0, 0], [hits[1], None, None], [hits[0], None, None])
    ar.check_properties(hits, 3, 4, labels, 0, want)
    for at, q, wrong in ((0, 0, 1), (0, 1, 3), (1, 0, 3), (1, 2, 1), (2, 0, 4), (3, 0, 1), (4, 0, hits[0]), (4, 0, hits[2]), (4, 0, hits[3]), (4, 1, hits[4]),
                         (5, 0, None), (5, 0, hits[3]), (5, 0, hits[2]), (5, 1, hits[4])):
        bad = [list(x) for x in want]
        bad[at][q] = wrong
        with pytest.raises(AssertionError):
            ar.check_properties(hits, 3, 4, labels, 0, bad)
    text = ar.render(["qa", "qb", "qc"], ["r0", "r1", "r2", "r3"], labels, want, {(0, 0): (0.5, 0.25), (0, 2): (0.125, 0.75)})
    assert text == "qa\tr3\tr0\t25|50|50\t0.500000\t0.250000\t2\t3\t4\tr1\t0.750000\nqb\t-\t-\t-\t-\t-\t0\t0\t1\t-\t-\nqc\t-\t-\t-\t-\t-\t0\t0\t0\t-\t-\n"
    assert ar.novel(["qa", "qb", "qc"], want) == "qb\nqc\n"


# ---- rk_assign_hits -------------------------------------------------------------------------------------------------------
def test_assign_hits_equals_the_reference_on_random_record_lists():
    rng = np.random.default_rng(131)
    ties = seconds = unanchored = strangers = 0
    for case in range(300):
        n_q, n_r, metric = int(rng.integers(1, 9)), int(rng.integers(1, 13)), case % 2
        hits, labels = random_hits(rng, n_q, n_r), random_labels(rng, n_r)
        rec = records(hits)
        got = capi.assign_hits(rec, n_q, n_r, labels, metric)
        assert [a.dtype for a in got] == [np.uint32] * 4 + [capi.HIT_DTYPE] * 2
        want = ar.assign(hits, n_q, n_r, labels, metric)
        assert as_ref(got) == list(want)
        ar.check_properties(hits, n_q, n_r, labels, metric, as_ref(got))
        by_pair = {(int(r["row"]), int(r["col"])): r for r in rec}
        for arr in got[4:]:   # the caller's records, unchanged: the marks in jorc and dist travel
            for r in arr[arr["row"] != NONE]:
                assert r == by_pair[(int(r["row"]), int(r["col"]))]
        bare = capi.assign_hits(rec, n_q, n_r, labels, metric, records=False)   # no record arrays: the same labels and counts
        assert bare[4] is None and bare[5] is None and same(bare[:4], got[:4])
        assert same(capi.assign_hits(rec[rng.permutation(len(rec))], n_q, n_r, labels, metric), got)   # the order of the hits does not matter
        for q in range(n_q):
            for best, group in ((want[4][q], True), (want[5][q], False)):
                if best is not None:
                    ties += sum(h[0] == q and labels[h[1]] != NONE and (labels[h[1]] == want[0][q]) == group and ar.cross(h, best, metric) == 0 for h in hits) > 1
            seconds += want[5][q] is not None
            unanchored += want[0][q] == NONE and want[1][q] > 0
            strangers += want[0][q] != NONE and labels[want[0][q]] != want[0][q]
    assert ties > 100 and seconds > 300 and unanchored > 50 and strangers > 100


def test_equal_ratios_from_different_counts_go_to_the_smaller_reference():
    for metric, a, b in ((0, (25, 50, 50), (20, 40, 40)), (1, (25, 50, 60), (20, 40, 70))):
        for first, second in ((a, b), (b, a)):   # under both index orders of the pair
            hits = [(0, 5) + second, (0, 2) + first]
            got = as_ref(capi.assign_hits(records(hits), 1, 6, [0, 0, 4, 0, 0, 1], metric))
            assert got == [[4], [2], [2], [1], [hits[1]], [hits[0]]]
            got = as_ref(capi.assign_hits(records(hits), 1, 6, [0, 0, 1, 0, 0, 4], metric))
            assert got == [[1], [2], [2], [1], [hits[1]], [hits[0]]]


def test_all_unlabelled_and_one_label():
    rng = np.random.default_rng(7)
    hits = random_hits(rng, 6, 9)
    assert len(hits) > 10
    got = as_ref(capi.assign_hits(records(hits), 6, 9, [NONE] * 9, 0))
    assert got[0] == [NONE] * 6 and got[2] == got[3] == [0] * 6 and got[4] == got[5] == [None] * 6
    assert got[1] == [sum(h[0] == q for h in hits) for q in range(6)] and sum(got[1]) == len(hits)
    got = as_ref(capi.assign_hits(records(hits), 6, 9, [8] * 9, 1))
    assert got == list(ar.assign(hits, 6, 9, [8] * 9, 1))
    assert got[1] == got[2] == got[3] and got[5] == [None] * 6 and all((l == 8) == (n > 0) for l, n in zip(got[0], got[1]))
    empty = capi.assign_hits(records([]), 3, 2, [0, 1], 0)   # no hit: every query novel
    assert as_ref(empty) == [[NONE] * 3, [0] * 3, [0] * 3, [0] * 3, [None] * 3, [None] * 3]


def test_assign_hits_refusals_write_nothing():
    L = capi.lib()
    L.rk_assign_hits.argtypes = HITS_ARGTYPES
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)])
    labels = np.array([0, 0, 2, NONE], dtype=np.uint32)
    out = marked(3)
    g = capi._assign_struct(out)
    for bad, code in (((3, 1, 25, 50, 50), RK_ERR_ARG),             # a query beyond n_query
                      ((0, 4, 25, 50, 50), RK_ERR_ARG),             # a reference beyond n_ref
                      ((0, 2, 0, 50, 50), RK_ERR_UNSUPPORTED),      # common = 0
                      ((0, 2, 51, 50, 50), RK_ERR_UNSUPPORTED),     # common > u (metric 1)
                      ((0, 2, -1, 50, 50), RK_ERR_UNSUPPORTED)):
        rec = records([(0, 1, 25, 50, 50), bad])
        assert L.rk_assign_hits(rec.ctypes.data, 2, 3, 4, labels.ctypes.data, 1, C.byref(g)) == code
        with pytest.raises(capi.RkError) as e:
            capi.assign_hits(rec, 3, 4, labels, 1)
        assert e.value.code == code
    for lab in ([0, 0, 2, 4], [0, 0, 2, NONE - 1]):   # a label that names no cluster
        arr = np.array(lab, dtype=np.uint32)
        assert L.rk_assign_hits(good.ctypes.data, 2, 3, 4, arr.ctypes.data, 0, C.byref(g)) == RK_ERR_ARG
    assert L.rk_assign_hits(good.ctypes.data, 2, 3, 4, None, 0, C.byref(g)) == RK_ERR_ARG
    assert L.rk_assign_hits(None, 2, 3, 4, labels.ctypes.data, 0, C.byref(g)) == RK_ERR_ARG
    assert L.rk_assign_hits(good.ctypes.data, 2, 3, 4, labels.ctypes.data, 0, None) == RK_ERR_ARG
    for k in range(4):
        part = list(out)
        part[k] = None
        lone = capi._assign_struct(part)
        assert L.rk_assign_hits(good.ctypes.data, 2, 3, 4, labels.ctypes.data, 0, C.byref(lone)) == RK_ERR_ARG
    assert untouched(out)   # refused before anything is written
    assert L.rk_assign_hits(good.ctypes.data, 2, 3, 4, labels.ctypes.data, 0, C.byref(g)) == 0
    assert out[0].tolist() == [0, NONE, NONE] and out[1].tolist() == [1, 0, 1] and out[2].tolist() == [1, 0, 0] and out[3].tolist() == [1, 0, 0]
    assert out[4]["row"].tolist() == [0, NONE, NONE] and out[5]["col"].tolist() == [NONE] * 3
    assert L.rk_assign_hits(None, 0, 0, 0, None, 0, C.byref(capi.AssignQueries())) == 0   # no query: nothing to write
    # a row that equals its column is an ordinary record here: query 1 against reference 1
    assert as_ref(capi.assign_hits(records([(1, 1, 25, 50, 50)]), 2, 2, [0, 0], 0))[0] == [NONE, 0]


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_assign_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_assign_rows.argtypes = ROWS_ARGTYPES
    opts = capi.DistOpts(0, 0, 20, 0, 0.05, 0, 1)
    out = marked(4)
    g, st = capi._assign_struct(out), capi.AssignStats()
    labels = np.zeros(4, dtype=np.uint32)
    assert L.rk_assign_rows(None, None, None, C.byref(opts), labels.ctypes.data, C.byref(g), C.byref(st)) == RK_ERR_ARG
    assert L.rk_assign_rows(None, None, None, None, None, None, None) == RK_ERR_ARG
    assert untouched(out)


def test_assign_symbols_are_exported():
    L = capi.lib()
    for name in ("rk_assign_rows", "rk_assign_hits"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.assign_rows) and callable(capi.assign_hits)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_ASSIGN 12\b", hdr)
    assert re.search(r"#define RK_ASSIGN_NONE 0xFFFFFFFFu\b", hdr) and capi.ASSIGN_NONE == ar.NONE == capi.DBSCAN_NOISE == 0xFFFFFFFF


def test_assign_structures_have_the_headers_sizes():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    width = {"uint64_t": 8, "uint32_t": 4, "rk_hit": 8}   # (the members of rk_assign_queries are pointers)

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for t, names in re.findall(r"\b(uint64_t|uint32_t|rk_hit)\s+([\w\s,*]+);", body):
            out += [(t, x.strip().lstrip("*")) for x in names.split(",")]
        return out
    st = fields("rk_assign_stats")
    assert [x for _, x in st] == [x for x, _ in capi.AssignStats._fields_] == ["edges", "borderline", "borderline_kept", "join_attempts", "border_attempts",
                                                                              "placed", "novel", "ambiguous", "sweeps"]
    assert C.sizeof(capi.AssignStats) == sum(width[t] for t, _ in st) == 48
    qs = fields("rk_assign_queries")
    assert [x for _, x in qs] == [x for x, _ in capi.AssignQueries._fields_] == ["label", "n_within", "n_labelled", "n_same", "nearest", "runner_up"]
    assert C.sizeof(capi.AssignQueries) == 48
