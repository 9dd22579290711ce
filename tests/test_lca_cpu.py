"""The host side of the classification by per-hash LCA (rk_lca_lists, rk_lca_call), the refusals that need no context and the sizes of
the structures -- against tests/_lca_ref.py: the rule twice in plain Python, the two statements checked against each other first, the
call's reference against what singles its result out.  All comparisons are exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _lca_ref as lr
from conftest import ROOT
from rabbitkssd_amd import capi
from rabbitkssd_amd.build import HIPCC

RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
NONE = lr.NONE


def library(refs, taxa, parent, queries, **sel):
    """rk_lca_lists over the exported lists: the rows as _lca_ref states them (unselected rows: empty, counts None), and the stats"""
    hashes, postings, counts = lr.exported(refs)
    rows = set(lr.selected_rows(len(queries), **sel))
    q_off, ql = lr.q_lists(hashes, queries)
    off, recs, matched, unl, st = capi.lca_lists(postings, counts, q_off, ql, taxa, parent, **sel)
    assert off.dtype == np.uint64 and off[0] == 0 and off[-1] == len(recs) and recs.dtype == capi.LCA_COUNT_DTYPE
    r = lr.records_of(recs)
    return [(r[int(off[i]):int(off[i + 1])], int(matched[i]) if i in rows else None, int(unl[i]) if i in rows else None) for i in range(len(queries))], st


def checked(refs, taxa, parent, queries):
    want = lr.from_sets(refs, taxa, parent, queries)
    got, st = library(refs, taxa, parent, queries)
    assert got == want, (parent, refs, taxa)
    for recs, matched, unl in got:
        assert sum(d for _, d in recs) + unl == matched and [t for t, _ in recs] == sorted(set(t for t, _ in recs))
    assert st["path"] == 2 and st["attempts"] == 1 and st["rows"] == len(queries) and st["records"] == sum(len(r) for r, _, _ in want)
    assert st["matched"] == sum(m for _, m, _ in want) and st["unlabelled"] == sum(u for _, _, u in want)
    assert st["lists"] == len(lr.exported(refs)[0]) and st["postings"] == sum(len(r) for r in refs)
    assert st["lane_lists"] + st["wave_lists"] + st["block_lists"] == st["lists"] and st["lane_max"] < st["wave_max"] < st["chunk"]
    return got


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def test_every_taxonomy_of_up_to_four_nodes_is_seen():
    seen = [0] * 5
    for parent in lr.taxonomies(4):
        seen[len(parent)] += 1
        assert lr.is_taxonomy(parent) and all(lr.root_path(parent, t)[-1] == lr.root_of(parent) for t in range(len(parent)))
    assert seen == [0, 1, 2, 9, 64]
    assert not lr.is_taxonomy([1, 0]) and not lr.is_taxonomy([0, 1]) and not lr.is_taxonomy([0, 2, 1]) and not lr.is_taxonomy([0, 5])


def test_the_two_statements_agree_on_every_small_case():
    """every taxonomy of up to 4 nodes, under each every labelling (NONE included) of up to 3 references -- the collections of
    _lca_ref.COLLECTIONS, in which every set of holders occurs as a posting list -- and the queries over a universe of 4 hashes"""
    seen = 0
    for parent, refs, taxa in lr.small_cases():
        assert lr.from_sets(refs, taxa, parent, lr.QUERIES) == lr.from_lists(*lr.exported(refs), taxa, parent, lr.QUERIES), (parent, refs, taxa)
        seen += 1
    assert seen == lr.N_SMALL_CASES == 19482 and len(lr.QUERIES) == 18


def test_reference_on_a_case_worked_by_hand():
    """      0            references: A in 3, B in 4, C in 2, D unlabelled
            / \\           hash 10: A        -> 3        hash 20: A, B  -> 1       hash 30: A, C -> 0
           1   2          hash 40: D        -> no labelled holder               hash 50: B, D -> 4 (D is ignored)
          / \\             hash 60: nobody
         3   4            query [10, 20, 20, 30, 40, 50, 60]: 3: 1, 1: 2, 0: 1, 4: 1; matched 6, unlabelled 1"""
    parent = [0, 0, 0, 1, 1]
    A, B, C_, D = [10, 20, 30], [20, 50], [30], [40, 50]
    taxa = [3, 4, 2, NONE]
    query = [10, 20, 20, 30, 40, 50, 60]
    want = [([(0, 1), (1, 2), (3, 1), (4, 1)], 6, 1)]
    assert lr.from_sets([A, B, C_, D], taxa, parent, [query]) == want
    assert lr.from_lists(*lr.exported([A, B, C_, D]), taxa, parent, [query]) == want
    assert checked([A, B, C_, D], taxa, parent, [query, [], [60], [40, 40]]) == want + [([], 0, 0), ([], 0, 0), ([], 2, 2)]
    # the call: scores 0: 1, 1: 3, 2: 1, 3: 4, 4: 4 -- 3 and 4 tie, their LCA 1 is the candidate; clade(1) = 4 of 5 retained
    recs = want[0][0]
    assert lr.call(recs, parent, (1, 0, 1, 0))[0] == dict(taxon=1, candidate=1, clade=4, score=4, retained=5, n_taxa=4)
    assert lr.call(recs, parent, (1, 4, 5, 0))[0]["taxon"] == 1 and lr.call(recs, parent, (1, 5, 6, 0))[0]["taxon"] == 0
    assert lr.call(recs, parent, (1, 5, 7, 1), 7)[0]["taxon"] == 0 and lr.call(recs, parent, (1, 6, 7, 1), 7)[0] == dict(
        taxon=NONE, candidate=1, clade=5, score=4, retained=5, n_taxa=4)
    assert lr.call(recs, parent, (2, 1, 1, 0)) == (dict(taxon=1, candidate=1, clade=2, score=2, retained=2, n_taxa=1), [2, 2, 0, 0])
    assert lr.call(recs, parent, (3, 0, 1, 0))[0] == dict(taxon=NONE, candidate=NONE, clade=0, score=0, retained=0, n_taxa=0)
    got = capi.lca_call(np.array(recs, dtype=capi.LCA_COUNT_DTYPE), [0, 4], parent, (1, 0, 1, 0), clades=True)
    assert got[0].tolist() == [(1, 1, 4, 4, 5, 4)] and got[1].tolist() == [5, 4, 1, 1]


def test_the_calls_reference_has_the_properties_that_single_it_out():
    seen = 0
    for parent, tallies in lr.small_tallies():
        T = len(parent)
        for recs in tallies:
            seen += 1
            total = sum(d for _, d in recs)
            for m in (1, 2):
                kept = [t for t, d in recs if d >= m]
                # {m, 1, 1, 0}: the LCA of the retained taxa
                c, _ = lr.call(recs, parent, (m, 1, 1, 0))
                assert c["taxon"] == (lr.lca_by_paths(parent, kept) if kept else NONE)
                # {m, 0, 1, *}: the candidate
                c0, _ = lr.call(recs, parent, (m, 0, 1, 0))
                assert c0["taxon"] == c0["candidate"] == lr.call(recs, parent, (m, 0, 1, 1), total + 3)[0]["taxon"]
                # raising P / Q moves the call to an ancestor or nowhere; the call passes, its child towards the candidate does not
                for w, size in ((0, 0), (1, total + 3)):
                    before = c0["candidate"]
                    for n, d in ((1, 3), (1, 2), (2, 3), (1, 1)):
                        c, _ = lr.call(recs, parent, (m, n, d, w), size)
                        D = size if w else c["retained"]
                        if before == NONE:
                            assert c["taxon"] == NONE
                        elif c["taxon"] != NONE:
                            assert lr.is_ancestor(parent, c["taxon"], before) and c["clade"] * d >= n * D
                            down = [t for t in lr.root_path(parent, c["candidate"]) if parent[t] == c["taxon"] and t != c["taxon"]]
                            if down:
                                below = sum(dd for t, dd in recs if dd >= m and lr.is_ancestor(parent, down[0], t))
                                assert below * d < n * D
                        else:
                            assert c["clade"] * d < n * D    # the root fails too
                        before = c["taxon"]
    assert seen == lr.N_SMALL_TALLIES == 5796 and T == 4


# ---- rk_lca_lists -------------------------------------------------------------------------------------------------------------------
def test_lca_lists_equals_the_reference_on_every_small_case():
    seen = 0
    for parent, refs, taxa in lr.small_cases():
        checked(refs, taxa, parent, lr.QUERIES)
        seen += 1
    assert seen == 19482


def random_case(rng):
    T = int(rng.integers(1, 12))
    order = rng.permutation(T)
    parent = [0] * T
    for k, t in enumerate(order):
        parent[t] = int(order[rng.integers(0, k)]) if k else int(t)
    n = int(rng.integers(0, 9))
    universe = [int(x) for x in rng.integers(0, 1 << 24, size=int(rng.integers(4, 40)))]
    pick = lambda m: [universe[int(i)] for i in rng.integers(0, len(universe), size=m)]   # noqa: E731  (repeats happen, on both sides)
    refs = [pick(int(rng.integers(0, 20))) for _ in range(n)]
    taxa = [NONE if rng.integers(0, 5) == 0 else int(rng.integers(0, T)) for _ in range(n)]
    queries = [pick(int(rng.integers(0, 30))) + [int(x) for x in rng.integers(0, 1 << 24, size=int(rng.integers(0, 4)))] for _ in range(int(rng.integers(0, 6)))]
    return parent, refs, taxa, queries


def test_lca_lists_equals_the_reference_on_random_collections():
    rng = np.random.default_rng(2026)
    inner = unl = multi = 0
    for case in range(400):
        parent, refs, taxa, queries = random_case(rng)
        assert lr.is_taxonomy(parent)
        got = checked(refs, taxa, parent, queries)
        assert got == lr.from_lists(*lr.exported(refs), taxa, parent, queries)
        leaves = set(range(len(parent))) - set(parent)
        inner += any(t not in leaves and t not in taxa for r, _, _ in got for t, _ in r)
        unl += any(u for _, _, u in got)
        multi += any(d > 1 for r, _, _ in got for _, d in r)
    assert inner > 50 and unl > 50 and multi > 50


def test_lca_lists_row_shards_concatenate_and_leave_the_rest_alone():
    rng = np.random.default_rng(5)
    for case in range(40):
        parent, refs, taxa, queries = random_case(rng)
        queries = (queries + [[1], [], [2, 2]])[:7]
        whole, _ = library(refs, taxa, parent, queries)
        for block in (1, 2):
            parts = [library(refs, taxa, parent, queries, row_first=k, row_step=3, row_block=block) for k in range(3)]
            for i in range(len(queries)):
                owner = (i // block) % 3
                for k, (rows, st) in enumerate(parts):
                    assert rows[i] == (whole[i] if k == owner else ([], None, None))
            assert sum(st["rows"] for _, st in parts) == len(queries)


# ---- rk_lca_call --------------------------------------------------------------------------------------------------------------------
def test_lca_call_equals_the_reference_on_every_small_tally():
    seen = 0
    for parent, tallies in lr.small_tallies():
        counts = np.array([r for recs in tallies for r in recs], dtype=capi.LCA_COUNT_DTYPE)
        off = np.cumsum([0] + [len(recs) for recs in tallies])
        sizes = [sum(d for _, d in recs) + 3 * (k % 2) for k, recs in enumerate(tallies)]
        for rule in lr.RULES:
            called, clade = capi.lca_call(counts, off, parent, rule, query_sizes=sizes, clades=True)
            for k, recs in enumerate(tallies):
                want, want_clade = lr.call(recs, parent, rule, sizes[k])
                assert dict(zip(called.dtype.names, called[k].tolist())) == want, (parent, recs, rule)
                assert clade[int(off[k]):int(off[k + 1])].tolist() == want_clade
        seen += len(tallies)
    assert seen == 5796 and len(lr.RULES) == 16


def test_lca_call_on_a_long_path_and_records_in_any_order():
    parent = lr.path(200_000)                       # no recursion anywhere: a path of 200,000 nodes
    recs = np.array([(199_999, 2), (5, 1), (100_000, 3)], dtype=capi.LCA_COUNT_DTYPE)
    called, clade = capi.lca_call(recs, [0, 3], parent, (1, 1, 2, 0), clades=True)
    assert called[0].tolist() == (100_000, 199_999, 5, 6, 6, 3) and clade.tolist() == [2, 6, 5]
    assert capi.lca_call(recs, [0, 3], parent, (1, 1, 1, 0))[0]["taxon"] == 5
    assert capi.lca_call(recs, [0, 3], parent, (1, 1, 1, 1), query_sizes=[7])[0]["taxon"] == NONE


def test_lca_call_refusals_write_nothing():
    parent = [0, 0, 1]
    recs = np.array([(1, 2), (2, 1)], dtype=capi.LCA_COUNT_DTYPE)
    L = capi.lib()
    L.rk_lca_call.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(capi.LcaRule), C.c_void_p, C.c_void_p]
    par = np.array(parent, dtype=np.uint32)
    off = np.array([0, 2], dtype=np.uint64)
    sizes = np.array([9], dtype=np.uint32)
    called = np.full(1, 0x77, dtype=capi.LCA_CALLED_DTYPE)
    clade = np.full(2, 0x77, dtype=np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def call(c=recs, o=off, s=sizes, p=par, T=3, rule=(1, 0, 1, 0), out=called):
        r = capi.LcaRule(*rule) if rule is not None else None
        return L.rk_lca_call(ptr(c), ptr(o), 1, ptr(s), ptr(p), T, C.byref(r) if r is not None else None, ptr(out), ptr(clade))
    for rule in ((0, 0, 1, 0), (1, 0, 0, 0), (1, 2, 1, 0), (1, 0, 1, 2), None):
        assert call(rule=rule) == RK_ERR_ARG, rule
    assert call(s=None, rule=(1, 1, 2, 1)) == RK_ERR_ARG                                  # denom 1 needs the sizes
    for null in ("c", "o", "p", "out"):
        assert call(**{null: None}) == RK_ERR_ARG, null
    assert call(T=0) == RK_ERR_ARG
    assert call(p=np.array([0, 1, 1], dtype=np.uint32)) == RK_ERR_ARG                      # two roots
    assert call(p=np.array([1, 2, 0], dtype=np.uint32)) == RK_ERR_ARG                      # none (a cycle)
    assert call(p=np.array([0, 2, 1], dtype=np.uint32)) == RK_ERR_ARG                      # a cycle beside the root
    assert call(p=np.array([0, 3, 1], dtype=np.uint32)) == RK_ERR_ARG                      # a parent beyond the nodes
    assert call(c=np.array([(1, 2), (3, 1)], dtype=capi.LCA_COUNT_DTYPE)) == RK_ERR_ARG    # a taxon beyond the nodes
    assert call(c=np.array([(1, 2), (1, 1)], dtype=capi.LCA_COUNT_DTYPE)) == RK_ERR_ARG    # ... twice
    assert call(o=np.array([1, 2], dtype=np.uint64)) == RK_ERR_ARG
    big = np.array([(1, 0xFFFFFFFF), (2, 1)], dtype=capi.LCA_COUNT_DTYPE)                  # sums that 32 bits do not hold
    assert call(c=big) == RK_ERR_UNSUPPORTED and call(c=big, rule=(0xFFFFFFFF, 0, 1, 0)) == RK_ERR_UNSUPPORTED
    assert (called.view(np.uint32) == 0x77).all() and (clade == 0x77).all()
    assert call(c=np.array([(1, 0xFFFFFFFE), (2, 1)], dtype=capi.LCA_COUNT_DTYPE), s=None) == 0     # ... and sums that just fit
    assert called[0].tolist() == (2, 2, 1, 0xFFFFFFFF, 0xFFFFFFFF, 2) and clade.tolist() == [0xFFFFFFFF, 1]
    assert call(s=None) == 0 and called[0].tolist() == (2, 2, 1, 3, 3, 2) and clade.tolist() == [3, 1]
    with pytest.raises(capi.RkError) as e:
        capi.lca_call(recs, [0, 2], parent, (0, 0, 1, 0))
    assert e.value.code == RK_ERR_ARG
    assert len(capi.lca_call(np.zeros(0, capi.LCA_COUNT_DTYPE), [0], parent)) == 0


# ---- the refusals of rk_lca_lists ---------------------------------------------------------------------------------------------------------
def test_lca_lists_refusals_write_nothing():
    L = capi.lib()
    L.rk_lca_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                               C.POINTER(capi.LcaOpts), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(capi.LcaStats)]
    u32, u64 = (lambda x: np.array(x, dtype=np.uint32)), (lambda x: np.array(x, dtype=np.uint64))
    postings, counts, q_off, ql, taxa, parent = u32([0, 1, 1]), u32([2, 1]), u64([0, 2, 3]), u64([0, 0, 1]), u32([1, NONE]), u32([0, 0])
    off = np.full(3, 0x77, dtype=np.uint64)
    matched, unl = np.full(2, 0x77, dtype=np.uint32), np.full(2, 0x77, dtype=np.uint32)
    recs, n = C.c_void_p(0x1234), C.c_uint64(0x77)
    st = capi.LcaStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def call(p=postings, c=counts, qo=q_off, l=ql, nq=2, n_ref=2, t=taxa, par=parent, T=2, opts=True, o=off, r=C.byref(recs), nn=C.byref(n), m=matched, u=unl,
             s=C.byref(st)):
        op = capi.LcaOpts(0, 0, 0)
        return L.rk_lca_lists(ptr(p), ptr(c), 2, ptr(qo), ptr(l), nq, n_ref, ptr(t), ptr(par), T, C.byref(op) if opts else None, ptr(o), r, nn, ptr(m), ptr(u), s)
    for null in ("p", "c", "qo", "l", "t", "par", "o", "r", "nn", "m", "u"):
        assert call(**{null: None}) == RK_ERR_ARG, null
    assert call(opts=False) == RK_ERR_ARG and call(T=0) == RK_ERR_ARG
    assert call(par=u32([0, 1])) == RK_ERR_ARG and call(par=u32([1, 0])) == RK_ERR_ARG and call(par=u32([0, 2])) == RK_ERR_ARG
    assert call(par=u32([0, 2, 1]), T=3) == RK_ERR_ARG                                   # a cycle beside the root
    assert call(t=u32([2, NONE])) == RK_ERR_ARG                                          # a taxon that is no node
    assert call(qo=u64([1, 2, 3])) == RK_ERR_ARG and call(qo=u64([0, 3, 2])) == RK_ERR_ARG
    assert call(l=u64([0, 2, 1])) == RK_ERR_ARG and call(l=u64([1, 0, 1])) == RK_ERR_ARG   # a list beyond the lists; out of order
    assert call(p=u32([0, 2, 1])) == RK_ERR_ARG                                          # a posting beyond the references
    assert call(n_ref=2 ** 31, t=None) == RK_ERR_UNSUPPORTED and call(T=2 ** 31) == RK_ERR_UNSUPPORTED
    assert recs.value == 0x1234 and n.value == 0x77 and (off == 0x77).all() and (matched == 0x77).all() and (unl == 0x77).all() and st.path == 0x5A5A5A5A
    # the good call writes, with and without stats: list 0 is held by 0 (node 1) and 1 (unlabelled), list 1 by 1 alone
    assert call() == 0 and off.tolist() == [0, 1, 1] and matched.tolist() == [2, 1] and unl.tolist() == [0, 1] and n.value == 1 and st.path == 2
    assert np.frombuffer(C.string_at(recs.value, 8), dtype=capi.LCA_COUNT_DTYPE).tolist() == [(1, 2)]
    L.rk_free_host(recs)
    assert call(s=None) == 0
    L.rk_free_host(recs)
    with pytest.raises(capi.RkError) as e:
        capi.lca_lists(postings, counts, q_off, ql, taxa, [0, 1])
    assert e.value.code == RK_ERR_ARG
    # no query; no list; no labelled genome
    off, recs_, m, u, st_ = capi.lca_lists([], [], [0], [], [], [0])
    assert off.tolist() == [0] and len(recs_) == 0 and st_["rows"] == 0
    off, recs_, m, u, st_ = capi.lca_lists([], [], [0, 0, 0], [], [0], [0])
    assert off.tolist() == [0, 0, 0] and m.tolist() == [0, 0]
    off, recs_, m, u, st_ = capi.lca_lists(postings, counts, q_off, ql, [NONE, NONE], parent)
    assert off.tolist() == [0, 0, 0] and m.tolist() == [2, 1] and u.tolist() == [2, 1] and st_["unlabelled"] == 3


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_lca_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_lca_rows.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    off = np.full(2, 0x77, dtype=np.uint64)
    recs, n = C.c_void_p(0x1234), C.c_uint64(0x77)
    assert L.rk_lca_rows(None, None, None, None, None, 1, None, off.ctypes.data, C.byref(recs), C.byref(n), None, None, None) == RK_ERR_ARG
    assert recs.value == 0x1234 and n.value == 0x77 and (off == 0x77).all()


def test_lca_symbols_and_constants():
    L = capi.lib()
    for name in ("rk_lca_rows", "rk_lca_lists", "rk_lca_call"):
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert callable(capi.Context.lca_rows) and callable(capi.lca_lists) and callable(capi.lca_call)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_LCA 16\b", hdr) and capi.MS_LCA == 16
    assert re.search(r"#define RK_LCA_NONE 0xFFFFFFFFu", hdr) and capi.LCA_NONE == lr.NONE == 2 ** 32 - 1
    L.rk_ctx_last_ms.restype = C.c_double
    assert L.rk_ctx_last_ms(None, 16) == 0.0


def test_lca_structures_have_the_headers_sizes():
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
    for name, cls, size in (("rk_lca_opts", capi.LcaOpts, 12), ("rk_lca_rule", capi.LcaRule, 16), ("rk_lca_stats", capi.LcaStats, 128)):
        f = fields(name)
        assert [x for _, x in f] == [x for x, _ in cls._fields_], name
        assert C.sizeof(cls) == sum(width[t] for t, _ in f) == size, name
    for name, dtype, size in (("rk_lca_count", capi.LCA_COUNT_DTYPE, 8), ("rk_lca_called", capi.LCA_CALLED_DTYPE, 24)):
        f = fields(name)
        assert [x for _, x in f] == list(dtype.names) and dtype.itemsize == size and all(t == "uint32_t" for t, _ in f), name


# ---- the stand-alone check under the host sanitizers ----------------------------------------------------------------------------------
def test_lca_lists_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/lca_lists_check.cpp: rk_lca_lists and rk_lca_call against a plain restatement in a program of its own, host code under
    -fsanitize=address,undefined.  No GPU call is made."""
    exe = str(tmp_path / "lca_lists_check")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rabbitkssd_amd", "csrc"),
                        os.path.join(ROOT, "rabbitkssd_amd", "csrc", "rk_lca.hip"), "-x", "hip", os.path.join(ROOT, "tools", "lca_lists_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    e = {k: v for k, v in os.environ.items() if not k.startswith("RK_")}
    p = subprocess.run([exe], capture_output=True, text=True, env=e)
    assert p.returncode == 0 and p.stdout.startswith("lca_lists_check: ok"), (p.stdout + p.stderr)[-4000:]
    assert not any(m in p.stderr for m in ("AddressSanitizer", "runtime error", "LeakSanitizer"))
