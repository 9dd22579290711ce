"""The host side of the winner-take-all containment screen (rk_screen_lists), the refusals of rk_screen_rows that need no context and the
sizes of its structures -- against tests/_screen_ref.py: the rule twice in plain Python, the two statements checked against each other and
against the facts that follow from the rule first."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _gather_ref as ga
import _screen_ref as sr
from _screen_cases import LISTS_ARGTYPES
from conftest import ROOT
from rabbitkssd_amd import capi

RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OPTIONS = [(c, w) for c in (1, 2, 3) for w in (0, 1, 2)]


def in_reference_form(off, recs, matched, n_cand, claimed):
    assert off.dtype == np.uint64 and recs.dtype == capi.SCREEN_REC_DTYPE and matched.dtype == n_cand.dtype == claimed.dtype == np.uint32
    return off.tolist(), sr.rec_tuples(recs), matched.tolist(), n_cand.tolist(), claimed.tolist()


def library(refs, queries, min_common=1, min_won=0, sizes=None, rng=None, **rows):
    """rk_screen_lists over the exported lists, in the reference's form; with rng every list is shuffled"""
    p, c, q_off, q_lists = sr.exported(refs, queries)
    if rng is not None:
        at = 0
        for n in c:
            p[at:at + n] = [p[at + i] for i in rng.permutation(n)]
            at += n
    qs = [len(set(int(h) for h in q)) for q in queries]
    return in_reference_form(*capi.screen_lists(p, c, q_off, q_lists, len(refs), sr.sizes_of(refs, sizes), qs, min_common, min_won, **rows))


def wanted(refs, queries, min_common=1, min_won=0, sizes=None, rows=None):
    off, recs, matched, n_cand, claimed = sr.as_arrays(sr.fast(refs, queries, min_common, min_won, sizes), refs, queries, rows, sizes)
    return off, recs, matched, n_cand, claimed


SUBSETS = [[h + 3 for h in range(5) if m >> h & 1] for m in range(32)]


def literal_collections(n_ref):
    """every collection of n_ref references over 5 hashes, literally: a reference is a subset"""
    return [list(refs) for refs in itertools.product(SUBSETS, repeat=n_ref)]


def holder_collections(n_ref, n_hash=5):
    """Every collection of n_ref references and a query over a universe of n_hash hashes, up to what cannot matter: a query's result
    depends on the references through their intersections with the query and through their SIZES alone (which hashes a reference holds
    outside the query changes nothing, how many does) and counts hashes without naming them.  So the query is the first k hashes,
    k = 0 .. n_hash, a collection is the MULTISET of the k hashes' holder sets (the empty set: a hash nobody indexes) times, per
    reference, the NUMBER 0 .. n_hash - k of hashes it holds outside the query (the first of the rest).  The order of the references is
    kept: ties go by it.  Yields (refs, query)."""
    for k in range(n_hash + 1):
        for holders in itertools.combinations_with_replacement(range(1 << n_ref), k):
            inside = [[h + 3 for h in range(k) if holders[h] >> r & 1] for r in range(n_ref)]
            for outside in itertools.product(range(n_hash - k + 1), repeat=n_ref):
                yield [inside[r] + [k + 3 + e for e in range(outside[r])] for r in range(n_ref)], [h + 3 for h in range(k)]


def second_query(query):
    """another query of the same universe: every other hash of the first and one nobody indexes"""
    return query[::2] + [99]


N_BY_HOLDERS = {3: sum(len(list(itertools.combinations_with_replacement(range(8), k))) * (6 - k) ** 3 for k in range(6)),
                4: sum(len(list(itertools.combinations_with_replacement(range(16), k))) * (6 - k) ** 4 for k in range(6))}


def small_collections():
    """(refs, queries) for every collection of up to 4 references and 2 queries over a universe of 5 hashes: literally for up to 2
    references with every query (and every PAIR of queries for up to 1), by holder sets and sizes for 3 and 4"""
    for n_ref in (0, 1, 2):
        for refs in literal_collections(n_ref):
            yield refs, SUBSETS       # 32 queries at once: each stands for itself
    for n_ref in (0, 1):
        for refs in literal_collections(n_ref):
            for a in SUBSETS:
                yield refs, [a, SUBSETS[(len(a) * 7 + 3) % 32]]
            for b in SUBSETS:
                yield refs, [SUBSETS[31], b]
    for n_ref in (3, 4):
        for refs, query in holder_collections(n_ref):
            yield refs, [query, second_query(query)]


assert N_BY_HOLDERS == {3: 10192, 4: 189728}
N_SMALL = (1 + 32 + 1024) + 2 * 32 * (1 + 32) + N_BY_HOLDERS[3] + N_BY_HOLDERS[4]


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_the_two_statements_agree_and_the_facts_hold_on_every_small_collection():
    seen = 0
    for refs, queries in small_collections():
        seen += 1
        base = {}
        for min_common in (1, 2, 3):   # each statement tallies once per min_common; min_won only chooses the records of a tally
            a, b = sr.tallies_from_sets(refs, queries, min_common), sr.fast_tallies(refs, queries, min_common)
            for min_won in (0, 1, 2):
                ra = sr.records(a, min_won)
                assert ra == sr.records(b, min_won), (refs, queries, min_common, min_won)
                if min_won == 0:
                    base[min_common] = ra
                    sr.facts(refs, queries, ra, min_common, 0)
                else:
                    assert all(t[3] >= min_won for recs, _, _, _ in ra for t in recs) and [x[1:] for x in ra] == [x[1:] for x in base[min_common]]
        sizes = set(sr.sizes_of(refs))
        if len(sizes) == 1 and sizes != {0}:   # references of one size: the best candidate is the greedy cover's first pick
            for (recs, _, _, _), (picks, _, _, _) in zip(base[1], ga.fast(refs, queries, 1, 1)):
                assert bool(recs) == bool(picks)
                if picks:
                    top = max(recs, key=lambda t: (t[2], -t[1]))
                    assert (top[1], top[3]) == (picks[0][1], picks[0][4])
    assert seen == N_SMALL


def test_reference_on_a_case_worked_by_hand():
    """A (10 hashes, all in the query) B (7: 6 shared with A, one of its own in the query, all in it) C (3 of 4 in the query) D (1 of 1, a
    hash A holds too).  Containments: A 10/10, B 7/7, D 1/1, C 3/4.  A, B and D tie at 1: the larger size first -- A, B, D -- then C.
    A claims its 10, B what is left of its 7 (hash 10), D nothing (its hash is A's), C its 3."""
    A, B, C_, D = list(range(0, 10)), list(range(4, 11)), [20, 21, 22, 23], [5]
    query = list(range(0, 11)) + [20, 21, 22, 99]
    for f in (sr.from_sets, sr.fast):
        assert f([A, B, C_, D], [query]) == [([(0, 0, 10, 10), (0, 1, 7, 1), (0, 2, 3, 3), (0, 3, 1, 0)], 14, 4, 14)]
        assert f([A, B, C_, D], [query], 1, 1) == [([(0, 0, 10, 10), (0, 1, 7, 1), (0, 2, 3, 3)], 14, 4, 14)]
        assert f([A, B, C_, D], [query], 4) == [([(0, 0, 10, 10), (0, 1, 7, 1)], 14, 2, 11)]       # C and D are no candidates: 20..22 unclaimed
        assert f([D, B, C_, A], [query]) == [([(0, 0, 1, 0), (0, 1, 7, 1), (0, 2, 3, 3), (0, 3, 10, 10)], 14, 4, 14)]
        assert f([A, A], [A]) == [([(0, 0, 10, 10), (0, 1, 10, 0)], 10, 2, 10)]                    # equal ratio and size: the smaller index
        # with B half in the query its containment is 7/14 < C's 3/4: its hash 10 stays its own, the rest is A's
        assert f([A, B + list(range(30, 37)), C_], [query]) == [([(0, 0, 10, 10), (0, 1, 7, 1), (0, 2, 3, 3)], 14, 3, 14)]
        assert f([A], [[], [77]]) == [([], 0, 0, 0), ([], 0, 0, 0)]


# ---- rk_screen_lists ----------------------------------------------------------------------------------------------------------
def check_together(cases):
    """rk_screen_lists on several small collections in ONE call per option: collection i keeps its hashes to itself (+ 1000 i), its
    references and queries follow those of the collections before it -- a tie goes by the index, and the order within a collection is kept.
    The reference answers every collection on its own; its records move by the collection's first reference and first query."""
    refs_all, queries_all, first = [], [], []
    for i, (refs, queries) in enumerate(cases):
        first.append((len(refs_all), len(queries_all)))
        refs_all += [[h + 1000 * i for h in r] for r in refs]
        queries_all += [[h + 1000 * i for h in q] for q in queries]
    p, c, q_off, q_lists = sr.exported(refs_all, queries_all)
    rs, qs = sr.sizes_of(refs_all), [len(set(q)) for q in queries_all]
    for min_common in (1, 2, 3):
        every = [sr.records(sr.fast_tallies(refs, queries, min_common)) for refs, queries in cases]
        for min_won in (0, 1, 2):   # (min_won filters the records, as the test above has checked on the reference itself)
            off, recs, matched, n_cand, claimed = [0], [], [], [], []
            for (r0, q0), result in zip(first, every):
                for mine, m, k, w in result:
                    recs += [(q + q0, r + r0, common, won, rs[r + r0], qs[q + q0]) for q, r, common, won in mine if won >= min_won]
                    off.append(len(recs))
                    matched.append(m)
                    n_cand.append(k)
                    claimed.append(w)
            got = in_reference_form(*capi.screen_lists(p, c, q_off, q_lists, len(refs_all), rs, qs, min_common, min_won))
            assert got == (off, recs, matched, n_cand, claimed), (cases, min_common, min_won)


def test_screen_lists_equals_the_reference_on_every_small_collection():
    seen, together = 0, []
    for refs, queries in small_collections():
        seen += 1
        together.append((refs, queries))
        if len(together) == 64:
            check_together(together)
            together = []
    check_together(together)
    assert seen == N_SMALL
    refs, queries = [[3, 4], [3]], [[3, 4, 5]]   # and one collection alone, through the helpers the other tests use
    assert library(refs, queries, 1, 1) == wanted(refs, queries, 1, 1) == ([0, 1], [(0, 0, 2, 2, 2, 3)], [2], [2], [2])


def random_clades(rng, n_ref, n_query, universe):
    """clades of related references of mixed sizes, queries that are unions of a few of them plus foreign hashes"""
    refs = []
    while len(refs) < n_ref:
        core = rng.choice(universe, size=int(rng.integers(5, 40)), replace=False)
        for _ in range(int(rng.integers(1, 6))):
            keep = core[rng.random(len(core)) < rng.uniform(0.4, 1.0)]
            own = rng.choice(universe, size=int(rng.integers(0, 8)), replace=False)
            refs.append(np.unique(np.concatenate([keep, own])).tolist())
    refs = refs[:n_ref]
    queries = []
    for k in range(n_query):
        members = rng.choice(n_ref, size=1 + k % 4, replace=False)
        parts = [np.array(refs[m], dtype=np.int64)[rng.random(len(refs[m])) < 0.8] for m in members]
        queries.append(np.unique(np.concatenate(parts + [rng.integers(universe, 2 * universe, size=int(rng.integers(0, 6)))])).tolist())
    return refs, queries + [[], [2 * universe + 1]]


def test_screen_lists_equals_the_reference_on_random_clades():
    rng = np.random.default_rng(31)
    for trial in range(12):
        refs, queries = random_clades(rng, 60, 10, 400)
        for min_common, min_won in ((1, 0), (2, 1), (5, 3)):
            got = library(refs, queries, min_common, min_won, rng=rng if trial % 2 else None)   # the order within a list does not matter
            assert got == wanted(refs, queries, min_common, min_won)
            assert len(got[1]) > 5 or min_common == 5
        if trial < 3:
            a = sr.from_sets(refs, queries)
            assert a == sr.fast(refs, queries)
            sr.facts(refs, queries, a)


def two_nested(L, sa, sb, min_won=0):
    """the query hits L lists; reference 0 holds all of them, reference 1 all but the last; their sizes are the caller's"""
    postings = np.empty(2 * L - 1, dtype=np.uint32)
    postings[0:2 * L - 2:2] = 0
    postings[1:2 * L - 2:2] = 1
    postings[2 * L - 2] = 0
    counts = np.full(L, 2, dtype=np.uint32)
    counts[L - 1] = 1
    off, recs, matched, n_cand, claimed = capi.screen_lists(postings, counts, [0, L], np.arange(L, dtype=np.uint64), 2, [sa, sb], [L], 1, min_won)
    assert off.tolist() == [0, len(recs)] and matched.tolist() == claimed.tolist() == [L] and n_cand.tolist() == [2]
    return [(int(r["ref"]), int(r["common"]), int(r["won"]), int(r["size_ref"])) for r in recs]


@pytest.mark.parametrize("log_l,m", [(10, 1047551), (10, 1000003), (24, 63)])
def test_products_that_differ_by_one_near_the_limit_of_the_sizes(log_l, m):
    """common 2^k + 1 against 2^k with sizes just below 2^30 chosen so that the two 64-bit products differ by exactly 1, either way:
    (L - 1)(L m + 1) - L (m (L - 1) + 1) = -1 and (L - 1)(L m - 1) - L (m (L - 1) - 1) = +1.  At k = 10 the products pass 2^39 (a 32-bit
    product wraps, a float's 24 bits cannot tell them apart); at k = 24 they pass 2^53, where a double cannot either."""
    L = (1 << log_l) + 1
    for d, first_wins in ((1, True), (-1, False)):
        sa, sb = L * m + d, m * (L - 1) + d
        assert L <= sa < 2 ** 30 and L - 1 <= sb < 2 ** 30 and (L * sb - (L - 1) * sa == d) and L * sb > (2 ** 53 if log_l == 24 else 2 ** 39)
        want = [(0, L, L, sa), (1, L - 1, 0, sb)] if first_wins else [(0, L, 1, sa), (1, L - 1, L - 1, sb)]
        assert two_nested(L, sa, sb) == want
        assert two_nested(L, sa, sb, 1) == [w for w in want if w[2] >= 1]
        if log_l == 10:   # the reference agrees (it is too slow for 2^24 lists)
            refs = [list(range(L)), list(range(L - 1))]
            assert [(r, c, w, (sa, sb)[r]) for _, r, c, w in sr.fast(refs, [list(range(L))], sizes=[sa, sb])[0][0]] == want
            assert sr.from_sets(refs, [list(range(L))], sizes=[sa, sb]) == sr.fast(refs, [list(range(L))], sizes=[sa, sb])


def test_equal_ratios_go_to_the_larger_size_then_to_the_smaller_index():
    # X holds 2 of its 4 hashes in the query, Y 3 of its 6, Z 1 of its 2; all hold hash 1
    X, Y, Z = [1, 2, 50, 51], [1, 3, 4, 60, 61, 62], [1, 70]
    query = [1, 2, 3, 4]
    for order in itertools.permutations(range(3)):
        refs = [None] * 3
        for role, at in zip((X, Y, Z), order):
            refs[at] = role
        x, y, z = order
        want = sorted([(0, x, 2, 1, 4, 4), (0, y, 3, 3, 6, 4), (0, z, 1, 0, 2, 4)])   # hash 1 goes to Y, the largest of the three halves
        assert library(refs, [query]) == ([0, 3], want, [4], [3], [4]) == wanted(refs, [query])
    # equal ratio and equal size: P, Q, R hold 2 of their 4 hashes each, all hold hash 1; the smallest index takes it
    P, Q, R = [1, 2, 50, 51], [1, 3, 60, 61], [1, 4, 70, 71]
    for order in itertools.permutations(range(3)):
        refs = [None] * 3
        for role, at in zip((P, Q, R), order):
            refs[at] = role
        got = library(refs, [query])
        assert got == wanted(refs, [query]) and [t[3] for t in got[1]] == [2, 1, 1]
    # the sizes are the CALLER's: the same lists under other sizes give another winner
    assert [t[3] for t in library([P, Q, R], [query], sizes=[5, 4, 4])[1]] == [1, 2, 1]    # 2/4 = 2/4 > 2/5: index 1
    assert [t[3] for t in library([P, Q, R], [query], sizes=[8, 4, 3])[1]] == [1, 1, 2]    # 2/3 wins
    assert [t[3] for t in library([P, Q, R], [query], sizes=[4, 8, 8])[1]] == [2, 1, 1]


def test_row_shards_concatenate_and_leave_the_rest_alone():
    rng = np.random.default_rng(5)
    refs, queries = random_clades(rng, 50, 21, 300)
    whole = library(refs, queries, 2, 1)
    p, c, q_off, q_lists = sr.exported(refs, queries)
    qs = [len(set(q)) for q in queries]
    L = capi.lib()
    L.rk_screen_lists.argtypes = LISTS_ARGTYPES
    u32, u64 = (lambda x: np.array(x, dtype=np.uint32)), (lambda x: np.array(x, dtype=np.uint64))
    p, c, q_off, q_lists, rs, qsz = u32(p), u32(c), u64(q_off), u64(q_lists), u32(sr.sizes_of(refs)), u32(qs)
    for step, block in ((2, 1), (3, 4), (4, 2)):
        outs = [np.full(len(queries), 0xDEAD, dtype=np.uint32) for _ in range(3)]
        parts = []
        for first in range(step):
            rows = sr.selected_rows(len(queries), first, step, block)
            assert library(refs, queries, 2, 1, row_first=first, row_step=step, row_block=block) == wanted(refs, queries, 2, 1, rows=rows)
            before = [a.copy() for a in outs]
            off = np.zeros(len(queries) + 1, dtype=np.uint64)
            recs, n = C.c_void_p(), C.c_uint64()
            o = capi.ScreenOpts(2, 1, first, step, block)
            assert L.rk_screen_lists(p.ctypes.data, c.ctypes.data, len(c), q_off.ctypes.data, q_lists.ctypes.data, len(queries), len(refs), rs.ctypes.data,
                                     qsz.ctypes.data, C.byref(o), off.ctypes.data, C.byref(recs), C.byref(n), *[a.ctypes.data for a in outs]) == 0
            parts += sr.rec_tuples(capi._take_array(recs, n.value, capi.SCREEN_REC_DTYPE))
            for a, b in zip(outs, before):   # the entries of the unselected rows keep what they held
                assert all(a[q] == b[q] for q in range(len(queries)) if q not in rows)
        assert sorted(parts) == whole[1] and [a.tolist() for a in outs] == list(whole[2:])


def test_screen_lists_refusals_write_nothing():
    L = capi.lib()
    L.rk_screen_lists.argtypes = LISTS_ARGTYPES
    u32, u64 = (lambda x: np.array(x, dtype=np.uint32)), (lambda x: np.array(x, dtype=np.uint64))
    postings, counts, q_off, ql, rs, qsz = u32([0, 1, 1]), u32([2, 1]), u64([0, 2, 3]), u64([0, 1, 1]), u32([1, 2]), u32([2, 1])
    off = np.full(3, 0x77, dtype=np.uint64)
    outs = [np.full(2, 0x77, dtype=np.uint32) for _ in range(3)]
    recs, n = C.c_void_p(0x1234), C.c_uint64(0x77)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def call(p=postings, c=counts, qo=q_off, l=ql, nq=2, n_ref=2, s=rs, z=qsz, opts=(1, 0, 0, 0, 0), o=off, r=C.byref(recs), nn=C.byref(n), m=outs[0], k=outs[1],
             w=outs[2]):
        op = capi.ScreenOpts(*opts) if opts is not None else None
        return L.rk_screen_lists(ptr(p), ptr(c), 2, ptr(qo), ptr(l), nq, n_ref, ptr(s), ptr(z), C.byref(op) if op is not None else None, ptr(o), r, nn, ptr(m),
                                 ptr(k), ptr(w))
    for null in ("p", "c", "qo", "l", "s", "z", "o", "r", "nn", "m", "k", "w"):
        assert call(**{null: None}) == RK_ERR_ARG, null
    assert call(opts=None) == RK_ERR_ARG and call(opts=(0, 0, 0, 0, 0)) == RK_ERR_ARG                # min_common == 0
    assert call(qo=u64([1, 2, 3])) == RK_ERR_ARG and call(qo=u64([0, 3, 2])) == RK_ERR_ARG
    assert call(l=u64([0, 2, 1])) == RK_ERR_ARG and call(l=u64([1, 0, 1])) == RK_ERR_ARG and call(l=u64([0, 0, 1])) == RK_ERR_ARG
    assert call(p=u32([0, 2, 1])) == RK_ERR_ARG                                                      # a posting beyond the references
    assert call(s=u32([1, 1])) == RK_ERR_ARG                                                         # reference 1 shares 2 hashes with query 0
    assert call(s=u32([1, 2 ** 30])) == RK_ERR_ARG and call(z=u32([2 ** 30, 1])) == RK_ERR_ARG       # a size of 2^30
    assert recs.value == 0x1234 and n.value == 0x77 and (off == 0x77).all() and all((a == 0x77).all() for a in outs)
    # the good call writes, at the largest size there is: list 0 is held by 0 and 1, list 1 by 1; 1/1 beats 2/(2^30 - 1)
    assert call(s=u32([1, 2 ** 30 - 1])) == 0 and off.tolist() == [0, 2, 3] and n.value == 3
    assert [a.tolist() for a in outs] == [[2, 1], [2, 1], [2, 1]]
    assert sr.rec_tuples(capi._take_array(recs, 3, capi.SCREEN_REC_DTYPE)) == [(0, 0, 1, 1, 1, 2), (0, 1, 2, 1, 2 ** 30 - 1, 2), (1, 1, 1, 1, 2 ** 30 - 1, 1)]
    # a reference of an UNSELECTED row may share more than its size: only the selected rows are read
    assert call(s=u32([1, 1]), opts=(1, 0, 1, 2, 1)) == 0
    L.rk_free_host(recs)
    with pytest.raises(capi.RkError) as e:
        capi.screen_lists(postings, counts, q_off, ql, 2, rs, qsz, min_common=0)
    assert e.value.code == RK_ERR_ARG
    with pytest.raises(ValueError):
        capi.screen_lists(postings, counts, q_off, ql, 3, rs, qsz)
    # no query; no list; no reference
    off, recs_, m, k, w = capi.screen_lists([], [], [0], [], 0, [], [])
    assert off.tolist() == [0] and len(recs_) == len(m) == 0
    off, recs_, m, k, w = capi.screen_lists([], [], [0, 0, 0], [], 2, [3, 4], [5, 0])
    assert off.tolist() == [0, 0, 0] and m.tolist() == k.tolist() == w.tolist() == [0, 0] and len(recs_) == 0


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_screen_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_screen_rows.argtypes = [C.c_void_p] * 11
    off = np.full(2, 0x77, dtype=np.uint64)
    recs, n = C.c_void_p(0x1234), C.c_uint64(0x77)
    o = capi.ScreenOpts(1, 0, 0, 0, 0)
    assert L.rk_screen_rows(None, None, None, C.byref(o), off.ctypes.data, C.byref(recs), C.byref(n), None, None, None, None) == RK_ERR_ARG
    assert L.rk_screen_rows(None, None, None, None, None, None, None, None, None, None, None) == RK_ERR_ARG
    assert recs.value == 0x1234 and n.value == 0x77 and (off == 0x77).all()


def test_screen_symbols_and_constants():
    L = capi.lib()
    for name in ("rk_screen_rows", "rk_screen_lists"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.screen_rows) and callable(capi.screen_lists)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_SCREEN 17\b", hdr) and capi.MS_SCREEN == 17
    L.rk_ctx_last_ms.restype = C.c_double
    assert L.rk_ctx_last_ms(None, 17) == 0.0


def test_screen_structures_have_the_headers_sizes():
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
    for name, cls, size in (("rk_screen_opts", capi.ScreenOpts, 20), ("rk_screen_stats", capi.ScreenStats, 120)):
        f = fields(name)
        assert [x for _, x in f] == [x for x, _ in cls._fields_], name
        assert C.sizeof(cls) == sum(width[t] for t, _ in f) == size, name
    f = fields("rk_screen_rec")
    assert [x for _, x in f] == list(capi.SCREEN_REC_DTYPE.names) == list(sr.REC_FIELDS) and capi.SCREEN_REC_DTYPE.itemsize == 24
    assert all(t == "uint32_t" for t, _ in f)


# ---- the stand-alone check under the host sanitizers ----------------------------------------------------------------------------------
def test_screen_lists_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/screen_lists_check.cpp: rk_screen_lists against a plain restatement in a program of its own, host code under
    -fsanitize=address,undefined.  No GPU call is made."""
    exe = str(tmp_path / "screen_lists_check")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"),
                        os.path.join(ROOT, "rabbitkssd_amd", "csrc", "rk_screen.hip"), "-x", "hip", os.path.join(ROOT, "tools", "screen_lists_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    p = subprocess.run([exe], capture_output=True, text=True, env=e)
    assert p.returncode == 0 and p.stdout.startswith("screen_lists_check: ok"), (p.stdout + p.stderr)[-4000:]
    assert not any(m in p.stderr for m in ("AddressSanitizer", "runtime error", "LeakSanitizer"))
