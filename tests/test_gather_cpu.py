"""The host side of the decomposition of queries into references (rk_gather_lists), the refusals of rk_gather_rows that need no context
and the sizes of its structures -- against tests/_gather_ref.py: the rule twice in plain Python, the two statements checked against each
other and against what singles the result out first."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _gather_ref as ga
from conftest import ROOT
from rabbitkssd_amd import capi

RK_ERR_ARG = -1
LISTS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(capi.GatherOpts),
                  C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p]
ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.GatherOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p,
                 C.c_void_p, C.c_void_p, C.POINTER(capi.GatherStats)]
OPTIONS = [(m, p) for m in (1, 2, 5) for p in (0, 1, 3)]


def exported(refs, queries, rng=None):
    """(postings, counts, q_off, q_lists, ref_sizes, query_sizes) of a collection and its queries as rk_index_export_lists returns the
    lists (by ascending hash) and as rk_gather_lists takes the queries; with rng every list is shuffled"""
    lists = ga.posting_lists(refs)
    hashes = sorted(lists)
    at = {h: i for i, h in enumerate(hashes)}
    if rng is not None:
        lists = {h: [v[i] for i in rng.permutation(len(v))] for h, v in lists.items()}
    postings = np.array([v for h in hashes for v in lists[h]], dtype=np.uint32)
    counts = np.array([len(lists[h]) for h in hashes], dtype=np.uint32)
    per = [sorted(at[h] for h in set(int(x) for x in q) if h in at) for q in queries]
    q_off = np.zeros(len(queries) + 1, dtype=np.uint64)
    q_off[1:] = np.cumsum([len(p) for p in per])
    q_lists = np.array([i for p in per for i in p], dtype=np.uint64)
    sizes = lambda xs: np.array([len(set(int(h) for h in x)) for x in xs], dtype=np.uint32)   # noqa: E731
    return postings, counts, q_off, q_lists, sizes(refs), sizes(queries)


def in_reference_form(off, picks, matched, n_cand, covered):
    assert off.dtype == np.uint64 and picks.dtype == capi.GATHER_PICK_DTYPE and matched.dtype == n_cand.dtype == covered.dtype == np.uint32
    return off.tolist(), ga.pick_tuples(picks), matched.tolist(), n_cand.tolist(), covered.tolist()


def library(refs, queries, min_new=1, max_picks=0, rng=None, **rows):
    """rk_gather_lists over the exported lists, in the reference's form"""
    p, c, q_off, q_lists, rs, qs = exported(refs, queries, rng)
    return in_reference_form(*capi.gather_lists(p, c, q_off, q_lists, len(refs), rs, qs, min_new, max_picks, **rows))


def literal_collections(n_ref, n_hash=5):
    """every collection of n_ref references over n_hash hashes, literally: a reference is a subset"""
    subsets = [[h + 3 for h in range(n_hash) if m >> h & 1] for m in range(1 << n_hash)]
    return [list(refs) for refs in itertools.product(subsets, repeat=n_ref)]


SUBSETS = [[h + 3 for h in range(5) if m >> h & 1] for m in range(32)]


def holder_collections(n_ref, n_hash=5):
    """Every collection of n_ref references and a query over a universe of n_hash hashes, up to what cannot matter: a query's result
    depends on the references through their intersections with the query alone (a hash outside the query changes nothing) and counts
    hashes without naming them (renaming the hashes changes nothing).  So the query is the first k hashes, k = 0 .. n_hash, and a
    collection is the MULTISET of the k hashes' holder sets (the empty set: a hash nobody indexes) -- C(2^n_ref + k - 1, k) per k, not
    2^(n_ref k).  The order of the references is kept: ties go by it.  Yields (refs, query)."""
    for k in range(n_hash + 1):
        for holders in itertools.combinations_with_replacement(range(1 << n_ref), k):
            yield [[h + 3 for h in range(k) if holders[h] >> r & 1] for r in range(n_ref)], [h + 3 for h in range(k)]


def second_query(query):
    """another query of the same universe: every other hash of the first and one nobody indexes"""
    return query[::2] + [99]


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_the_two_statements_agree_and_are_singled_out_on_every_small_collection():
    """every collection of up to 4 references and 2 queries over a universe of 5 hashes: literally for up to 2 references with every
    query (and every PAIR of queries for up to 1), by holder sets for 3 and 4 (holder_collections says why that loses nothing)"""
    def check(refs, queries):
        for min_new, max_picks in ((1, 0), (2, 0), (1, 2)):
            a = ga.from_sets(refs, queries, min_new, max_picks)
            assert a == ga.fast(refs, queries, min_new, max_picks), (refs, queries, min_new, max_picks)
            ga.singled_out(refs, queries, a, min_new, max_picks)
    seen = 0
    for n_ref in (0, 1, 2):
        for refs in literal_collections(n_ref):
            check(refs, SUBSETS)       # 32 queries at once: each stands for itself
            seen += 1
    for n_ref in (0, 1):
        for refs in literal_collections(n_ref):
            for a in SUBSETS:
                check(refs, [a, SUBSETS[(len(a) * 7 + 3) % 32]])
            for b in SUBSETS:
                check(refs, [SUBSETS[31], b])
    by_holders = 0
    for n_ref in (3, 4):
        for refs, query in holder_collections(n_ref):
            check(refs, [query, second_query(query)])
            by_holders += 1
    assert seen == 1 + 32 + 1024 and by_holders == 1287 + 20349


def test_reference_on_a_case_worked_by_hand():
    # A holds most of the query, B lies almost inside A, C is small and disjoint: by overlap the order is A B C, greedily A C (B)
    A, B, C_ = list(range(0, 10)), list(range(4, 11)), [20, 21, 22]
    query = list(range(0, 11)) + [20, 21, 22, 99]
    for f in (ga.from_sets, ga.fast):
        assert f([A, B, C_], [query]) == [([(0, 0, 0, 10, 10, 4), (0, 2, 1, 3, 3, 1), (0, 1, 2, 7, 1, 0)], 14, 3, 14)]
        assert f([A, B, C_], [query], 2) == [([(0, 0, 0, 10, 10, 4), (0, 2, 1, 3, 3, 1)], 14, 3, 13)]
        assert f([B, A, C_], [query], 1, 1) == [([(0, 1, 0, 10, 10, 4)], 14, 3, 10)]
        assert f([A, A], [A]) == [([(0, 0, 0, 10, 10, 0)], 10, 2, 10)]            # a tie: the smaller index, and nothing is left
        assert f([A], [[], [77]]) == [([], 0, 0, 0), ([], 0, 0, 0)]


# ---- rk_gather_lists ----------------------------------------------------------------------------------------------------------
def test_gather_lists_equals_the_reference_on_every_small_collection():
    """every collection of up to 4 references and 2 queries over a universe of 5 hashes, as above"""
    def check(refs, queries):
        for min_new, max_picks in ((1, 0), (2, 0), (1, 2)):
            want = ga.as_arrays(ga.from_sets(refs, queries, min_new, max_picks), refs, queries)
            assert library(refs, queries, min_new, max_picks) == want, (refs, queries, min_new, max_picks)
    seen = 0
    for n_ref in (0, 1, 2):
        for refs in literal_collections(n_ref):
            check(refs, SUBSETS)
            seen += 1
    for n_ref in (3, 4):
        for refs, query in holder_collections(n_ref):
            check(refs, [query, second_query(query)])
            seen += 1
    assert seen == 1 + 32 + 1024 + 1287 + 20349


def random_case(rng):
    n = int(rng.integers(1, 25))
    universe = int(rng.integers(8, 80))
    refs = [rng.integers(0, universe, size=int(rng.integers(0, 30))).tolist() for _ in range(n)]   # repeats happen: taken as sets
    queries = []
    for _ in range(int(rng.integers(1, 6))):
        members = rng.choice(n, size=int(rng.integers(0, min(n, 6) + 1)), replace=False)
        q = [h for m in members for h in refs[m]] + rng.integers(universe, universe + 20, size=int(rng.integers(0, 8))).tolist()   # + foreign hashes
        queries.append([int(h) for h in q])
    return refs, queries


def test_gather_lists_equals_the_reference_on_random_collections():
    rng = np.random.default_rng(313)
    ties = many = stopped = 0
    for case in range(150):
        refs, queries = random_case(rng)
        for min_new, max_picks in OPTIONS:
            result = ga.from_sets(refs, queries, min_new, max_picks)
            assert result == ga.fast(refs, queries, min_new, max_picks)
            ga.singled_out(refs, queries, result, min_new, max_picks)
            want = ga.as_arrays(result, refs, queries)
            assert library(refs, queries, min_new, max_picks) == want
            assert library(refs, queries, min_new, max_picks, rng) == want   # the order inside a list does not matter
            many += any(len(r[0]) > 3 for r in result)
            stopped += any(max_picks and len(r[0]) == max_picks for r in result)
        sets = [set(r) for r in refs]
        ties += any(len(set(q) & a) == len(set(q) & b) > 0 for q in queries for a, b in itertools.combinations(sets, 2))
    assert ties > 50 and many > 50 and stopped > 50


def test_row_shards_concatenate_to_the_whole():
    rng = np.random.default_rng(5)
    refs, _ = random_case(rng)
    queries = [rng.choice(80, size=12).tolist() for _ in range(11)]
    whole = library(refs, queries)
    for step, block in ((2, 1), (2, 3), (3, 2)):
        picks, matched, n_cand, covered = [], [0] * 11, [0] * 11, [0] * 11
        for first in range(step):
            rows = ga.selected_rows(11, first, step, block)
            off, p, m, c, v = library(refs, queries, row_first=first, row_step=step, row_block=block)
            assert (off, p, m, c, v) == ga.as_arrays(ga.from_sets(refs, queries), refs, queries, rows)
            picks += p
            for r in rows:
                matched[r], n_cand[r], covered[r] = m[r], c[r], v[r]
        assert (sorted(picks, key=lambda t: (t[0], t[2])), matched, n_cand, covered) == (whole[1], whole[2], whole[3], whole[4])


def test_lists_with_repeats_and_empty_lists():
    # list 0 names reference 1 three times: it counts once; list 1 is empty: it matches nothing
    postings = np.array([1, 1, 0, 1, 2], dtype=np.uint32)
    counts = np.array([4, 0, 1], dtype=np.uint32)
    off, picks, matched, n_cand, covered = capi.gather_lists(postings, counts, [0, 3], [0, 1, 2], 3, [5, 6, 7], [9])
    assert ga.pick_tuples(picks) == [(0, 0, 0, 1, 1, 1, 5, 9), (0, 2, 1, 1, 1, 0, 7, 9)] and off.tolist() == [0, 2]
    assert (matched.tolist(), n_cand.tolist(), covered.tolist()) == ([2], [3], [2])


def test_gather_lists_refusals_write_nothing():
    L = capi.lib()
    L.rk_gather_lists.argtypes = LISTS_ARGTYPES
    postings = np.array([0, 1, 1], dtype=np.uint32)
    counts = np.array([2, 1], dtype=np.uint32)
    q_off = np.array([0, 2, 2], dtype=np.uint64)
    q_lists = np.array([0, 1], dtype=np.uint64)
    rs, qs = np.array([2, 1], dtype=np.uint32), np.array([3, 0], dtype=np.uint32)
    off = np.full(3, 0x77, dtype=np.uint64)
    outs = [np.full(2, 0x55, dtype=np.uint32) for _ in range(3)]
    picks, n = C.c_void_p(0x1234), C.c_uint64(0xABAB)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def call(p=postings, c=counts, n_lists=2, qo=q_off, ql=q_lists, nq=2, n_ref=2, r=rs, q=qs, opts=(1, 0, 0, 0, 0), o=off, pk=C.byref(picks), nn=C.byref(n),
             m=outs[0], nc=outs[1], cv=outs[2]):
        op = capi.GatherOpts(*opts) if opts is not None else None
        return L.rk_gather_lists(ptr(p), ptr(c), n_lists, ptr(qo), ptr(ql), nq, n_ref, ptr(r), ptr(q), C.byref(op) if op is not None else None, ptr(o), pk, nn,
                                 ptr(m), ptr(nc), ptr(cv))
    assert call(opts=(0, 0, 0, 0, 0)) == RK_ERR_ARG                                 # min_new == 0
    assert call(opts=None) == RK_ERR_ARG
    assert call(p=np.array([0, 2, 1], dtype=np.uint32)) == RK_ERR_ARG               # a posting beyond the references
    assert call(qo=np.array([1, 2, 2], dtype=np.uint64)) == RK_ERR_ARG              # offsets that do not begin at 0
    assert call(qo=np.array([0, 2, 1], dtype=np.uint64)) == RK_ERR_ARG              # ... that descend
    assert call(ql=np.array([0, 2], dtype=np.uint64)) == RK_ERR_ARG                 # a list that does not exist
    assert call(ql=np.array([1, 0], dtype=np.uint64)) == RK_ERR_ARG                 # lists out of order
    assert call(ql=np.array([1, 1], dtype=np.uint64)) == RK_ERR_ARG                 # ... or twice
    for null in ("p", "c", "qo", "ql", "r", "q", "o", "m", "nc", "cv"):
        assert call(**{null: None}) == RK_ERR_ARG, null
    assert call(pk=None) == RK_ERR_ARG and call(nn=None) == RK_ERR_ARG
    assert picks.value == 0x1234 and n.value == 0xABAB and (off == 0x77).all() and all((a == 0x55).all() for a in outs)
    with pytest.raises(capi.RkError) as e:
        capi.gather_lists(postings, counts, q_off, q_lists, 2, rs, qs, min_new=0)
    assert e.value.code == RK_ERR_ARG
    assert call() == 0 and n.value == 1 and off.tolist() == [0, 1, 1] and outs[0].tolist() == [2, 0]   # and the good call writes
    L.rk_free_host(picks)
    # no query, no list, no reference: RK_OK, an offset table of one 0
    off, picks_, matched, n_cand, covered = capi.gather_lists(np.zeros(0, np.uint32), np.zeros(0, np.uint32), [0], [], 0, [], [])
    assert off.tolist() == [0] and len(picks_) == len(matched) == 0


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_gather_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_gather_rows.argtypes = ROWS_ARGTYPES
    picks, n = C.c_void_p(0x1234), C.c_uint64(0xABAB)
    off = np.full(3, 0x77, dtype=np.uint64)
    o, st = capi.GatherOpts(1, 0, 0, 0, 0), capi.GatherStats()
    assert L.rk_gather_rows(None, None, None, C.byref(o), off.ctypes.data, C.byref(picks), C.byref(n), None, None, None, C.byref(st)) == RK_ERR_ARG
    assert L.rk_gather_rows(None, None, None, None, None, None, None, None, None, None, None) == RK_ERR_ARG
    assert picks.value == 0x1234 and n.value == 0xABAB and (off == 0x77).all()


def test_gather_symbols_and_constants():
    L = capi.lib()
    for name in ("rk_gather_rows", "rk_gather_lists"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.gather_rows) and callable(capi.gather_lists)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_GATHER 14\b", hdr) and capi.MS_GATHER == 14
    L.rk_ctx_last_ms.restype = C.c_double
    assert L.rk_ctx_last_ms(None, 14) == 0.0


def test_gather_structures_have_the_headers_sizes():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    width = {"uint64_t": 8, "uint32_t": 4}

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for t, names in re.findall(r"\b(uint64_t|uint32_t)\s+([\w\s,]+);", body):
            out += [(t, x.strip()) for x in names.split(",")]
        return out
    st = fields("rk_gather_stats")
    assert [x for _, x in st] == [x for x, _ in capi.GatherStats._fields_]
    assert C.sizeof(capi.GatherStats) == sum(width[t] for t, _ in st) == 112
    op = fields("rk_gather_opts")
    assert [x for _, x in op] == [x for x, _ in capi.GatherOpts._fields_] == ["min_new", "max_picks", "row_first", "row_step", "row_block"]
    assert C.sizeof(capi.GatherOpts) == 20
    pk = fields("rk_gather_pick")
    assert [x for _, x in pk] == list(capi.GATHER_PICK_DTYPE.names) == list(ga.PICK_FIELDS) and capi.GATHER_PICK_DTYPE.itemsize == 32
