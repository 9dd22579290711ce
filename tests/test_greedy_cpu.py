"""The host side of the greedy representatives (rk_greedy_hits), the refusals of rk_greedy_rows that need no context and the size of
rk_greedy_stats -- against tests/_greedy_ref.py, the sequential rule with exact rational ratios, which is itself checked against the
properties that characterise its result."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _greedy_ref as gr
from rabbitkssd_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_ERR_ARG = -1
# (common, size0, size1) with the ratios 1/4, 2/4, 3/4, 20/60 and 25/75 under metric 0 (u = size0 + size1 - common); under metric 1
# (u = min) they read 20/50, 40/60, 60/70, 20/40 and 25/50: the last two tie there as well
TRIPLES = [(20, 50, 50), (40, 60, 60), (60, 70, 70), (20, 40, 40), (25, 50, 50)]
HITS_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]


def records(hits):
    rec = np.zeros(len(hits), dtype=capi.HIT_DTYPE)
    for k, h in enumerate(hits):
        rec[k] = (h[0], h[1], h[2], h[3], h[4], 0, 0.25 + k, 0.5 + k)   # (jorc and dist: marks that must travel unchanged)
    return rec


def random_graph(rng, n, triple_of):
    """a random subset of the pairs of n genomes, one record per pair"""
    pairs = list(itertools.combinations(range(n), 2))
    m = int(rng.integers(0, len(pairs) + 1)) if pairs else 0
    return [pairs[i] + triple_of(pairs[i]) for i in rng.choice(len(pairs), size=m, replace=False)] if m else []


def compare(hits, n, metric, priority, got_rep, got_links):
    rep, links = gr.greedy(hits, n, metric, priority)
    assert got_rep.dtype == np.uint32 and got_rep.tolist() == rep
    assert gr.hit_tuples(got_links) == [links[m] for m in sorted(links)]
    return rep, links


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_reference_has_the_characterising_properties():
    rng = np.random.default_rng(50)
    for case in range(300):
        n = int(rng.integers(1, 15))
        metric = case % 2
        hits = random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))])
        priority = rng.integers(0, 4, size=n) if case % 3 else rng.permutation(n)   # (few values: the index breaks ties)
        rep, links = gr.greedy(hits, n, metric, priority)
        gr.check_properties(hits, n, metric, rep, links, priority)
    # the checker does refuse: the middle of a path as a second representative, and a member sent to the farther representative
    path = [(0, 1, 25, 50, 50), (1, 2, 25, 50, 50)]
    with pytest.raises(AssertionError):
        gr.check_properties(path, 3, 0, [0, 1, 1], {2: path[1]}, [0, 1, 2])
    fork = [(0, 2, 20, 50, 50), (1, 2, 40, 60, 60)]
    assert gr.greedy(fork, 3, 0, [0, 1, 2]) == ([0, 1, 1], {2: fork[1]})
    with pytest.raises(AssertionError):
        gr.check_properties(fork, 3, 0, [0, 1, 0], {2: fork[0]}, [0, 1, 2])


def test_parallel_rounds_decide_what_the_sequential_rule_decides():
    rng = np.random.default_rng(53)
    most = 0
    for case in range(300):
        n = int(rng.integers(1, 15))
        hits = random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))])
        priority = rng.integers(0, 4, size=n) if case % 3 else rng.permutation(n)
        rep, _ = gr.greedy(hits, n, case % 2, priority)
        is_rep, count = gr.rounds(hits, n, priority)
        assert is_rep == [rep[i] == i for i in range(n)] and count <= n and (count > 0) == bool(hits)
        most = max(most, count)
    assert most >= 5
    n = 40   # a path laid in priority order: one genome per round; the same path walked from both ends inwards: half as many
    path = [(i, i + 1, 25, 50, 50) for i in range(n - 1)]
    is_rep, count = gr.rounds(path, n, list(range(n)))
    assert count == n and is_rep == [i % 2 == 0 for i in range(n)]
    assert gr.rounds(path, n, [min(i, n - 1 - i) for i in range(n)])[1] == n // 2


# ---- rk_greedy_hits -------------------------------------------------------------------------------------------------------
def test_greedy_hits_equals_the_reference_on_random_graphs():
    rng = np.random.default_rng(51)
    members = 0
    for case in range(400):
        n = int(rng.integers(1, 15))
        metric = case % 2
        hits = random_graph(rng, n, lambda pair: TRIPLES[int(rng.integers(len(TRIPLES)))])
        priority = rng.integers(0, 4, size=n) if case % 3 else rng.permutation(n)
        rec = records(hits)
        got_rep, got_links = capi.greedy_hits(rec, n, metric, priority)
        rep, links = compare(hits, n, metric, priority, got_rep, got_links)
        members += len(links)
        by_pair = {(int(r["row"]), int(r["col"])): r for r in rec}
        for link in got_links:   # the records travel unchanged
            assert link == by_pair[(int(link["row"]), int(link["col"]))]
        shuffled = rec[rng.permutation(len(rec))]   # the order of the hits does not matter
        again_rep, again_links = capi.greedy_hits(shuffled, n, metric, priority)
        assert np.array_equal(again_rep, got_rep) and np.array_equal(again_links, got_links)
    assert members > 400


def test_sizes_come_from_the_records_without_a_priority():
    rng = np.random.default_rng(52)
    for case in range(200):
        n = int(rng.integers(1, 15))
        metric = case % 2
        size = rng.choice([30, 40, 50, 60], size=n).tolist()   # few sizes: the index breaks ties
        hits = random_graph(rng, n, lambda pair: (int(rng.integers(1, min(size[pair[0]], size[pair[1]]) + 1)), size[pair[0]], size[pair[1]]))
        got_rep, got_links = capi.greedy_hits(records(hits), n, metric)
        rep, links = compare(hits, n, metric, None, got_rep, got_links)
        gr.check_properties(hits, n, metric, rep, links)
    # the larger sketch first: genome 2 is the representative, though 0 has the smallest index
    star = [(0, 2, 30, 40, 60), (1, 2, 30, 50, 60)]
    got_rep, got_links = capi.greedy_hits(records(star), 3, 0)
    assert got_rep.tolist() == [2, 2, 2] and gr.hit_tuples(got_links) == star
    assert capi.greedy_hits(records(star), 3, 0, [0, 1, 2])[0].tolist() == [0, 1, 0]   # (0 and 1 are not adjacent)


def test_ties_a_later_representative_and_an_empty_list():
    # 25/75 ties 20/60 under metric 0: the member goes to the smaller index, whichever of the two counts that is
    for a, b in (((0, 2, 25, 70, 30), (1, 2, 20, 50, 30)), ((0, 2, 20, 50, 30), (1, 2, 25, 70, 30))):
        got_rep, got_links = capi.greedy_hits(records([b, a]), 3, 0, [0, 0, 1])
        assert got_rep.tolist() == [0, 1, 0] and gr.hit_tuples(got_links) == [a]
    # R1 = 0, M = 1, R2 = 2 in priority order: M is nearer to R2, which comes later and is not considered
    hits = [(0, 1, 20, 50, 50), (1, 2, 60, 70, 70)]
    got_rep, got_links = capi.greedy_hits(records(hits), 3, 0, [0, 1, 2])
    assert got_rep.tolist() == [0, 0, 2] and gr.hit_tuples(got_links) == [hits[0]]
    got_rep, got_links = capi.greedy_hits(records(hits), 3, 0, [0, 2, 1])   # with R2 first in line it is taken
    assert got_rep.tolist() == [0, 2, 2] and gr.hit_tuples(got_links) == [hits[1]]
    for n in (0, 1, 7):
        got_rep, got_links = capi.greedy_hits(records([]), n, 0)
        assert got_rep.tolist() == list(range(n)) and len(got_links) == 0
    L = capi.lib()
    L.rk_greedy_hits.argtypes = HITS_ARGTYPES
    rep = np.full(5, 77, dtype=np.uint32)
    links, n_links = C.c_void_p(5), C.c_uint64(7)
    assert L.rk_greedy_hits(None, 0, 5, None, 0, rep.ctypes.data, C.byref(links), C.byref(n_links)) == 0   # a list of no hits may be NULL
    assert rep.tolist() == [0, 1, 2, 3, 4] and n_links.value == 0 and links.value is None


def test_greedy_hits_refusals():
    L = capi.lib()
    L.rk_greedy_hits.argtypes = HITS_ARGTYPES
    good = records([(0, 1, 25, 50, 50), (2, 3, 20, 40, 40)])
    rep = np.full(4, 77, dtype=np.uint32)
    links, n_links = C.c_void_p(), C.c_uint64()
    for bad in ([(0, 4, 25, 50, 50)], [(4, 5, 25, 50, 50)], [(1, 0xFFFFFFFF, 25, 50, 50)], [(2, 2, 25, 50, 50)]):
        both = np.concatenate([good, records(bad)])
        for priority in (None, np.arange(4, dtype=np.uint32)):
            p = priority.ctypes.data if priority is not None else None
            assert L.rk_greedy_hits(both.ctypes.data, 3, 4, p, 0, rep.ctypes.data, C.byref(links), C.byref(n_links)) == RK_ERR_ARG
            assert np.all(rep == 77)   # refused before anything is written
        with pytest.raises(capi.RkError) as e:
            capi.greedy_hits(both, 4, 0)
        assert e.value.code == RK_ERR_ARG
    # genome 1 with 50 hashes in one record and 40 in another: refused when the sizes are what orders the genomes
    odd = records([(0, 1, 25, 50, 50), (1, 2, 20, 40, 40)])
    assert L.rk_greedy_hits(odd.ctypes.data, 2, 4, None, 0, rep.ctypes.data, C.byref(links), C.byref(n_links)) == RK_ERR_ARG
    assert L.rk_greedy_hits(good.ctypes.data, 2, 4, None, 0, None, C.byref(links), C.byref(n_links)) == RK_ERR_ARG
    assert L.rk_greedy_hits(good.ctypes.data, 2, 4, None, 0, rep.ctypes.data, None, C.byref(n_links)) == RK_ERR_ARG
    assert L.rk_greedy_hits(good.ctypes.data, 2, 4, None, 0, rep.ctypes.data, C.byref(links), None) == RK_ERR_ARG
    assert L.rk_greedy_hits(None, 2, 4, None, 0, rep.ctypes.data, C.byref(links), C.byref(n_links)) == RK_ERR_ARG
    assert np.all(rep == 77)
    assert L.rk_greedy_hits(good.ctypes.data, 2, 4, None, 0, rep.ctypes.data, C.byref(links), C.byref(n_links)) == 0
    assert rep.tolist() == [0, 0, 2, 2] and n_links.value == 2
    L.rk_free_host(links)


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_greedy_rows_refuses_null_pointers_without_a_context():
    L = capi.lib()
    L.rk_greedy_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64), C.POINTER(capi.GreedyStats)]
    opts = capi.DistOpts(1, 0, 20, 0, 0.05, 0, 1)
    rep = np.zeros(4, dtype=np.uint32)
    links, n, st = C.c_void_p(), C.c_uint64(), capi.GreedyStats()
    assert L.rk_greedy_rows(None, None, C.byref(opts), None, rep.ctypes.data, C.byref(links), C.byref(n), C.byref(st)) == RK_ERR_ARG
    assert L.rk_greedy_rows(None, None, None, None, None, None, None, None) == RK_ERR_ARG


def test_greedy_symbols_are_exported():
    L = capi.lib()
    for name in ("rk_greedy_rows", "rk_greedy_hits"):
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None   # (ctypes raises AttributeError for a symbol the library lacks)
    assert callable(capi.Context.greedy_rows) and callable(capi.greedy_hits)
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    assert re.search(r"#define RK_MS_GREEDY_ROUNDS 7\b", hdr)


def test_greedy_stats_has_the_headers_size():
    hdr = open(os.path.join(ROOT, "include", "rabbitkssd.h")).read()
    m = re.search(r"typedef struct rk_greedy_stats \{(.*?)\} rk_greedy_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    width = {"uint64_t": 8, "uint32_t": 4}
    fields = [(t, name) for t, name in re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)]
    assert [name for _, name in fields] == [name for name, _ in capi.GreedyStats._fields_]
    assert [name for _, name in fields] == ["edges", "borderline", "borderline_kept", "join_attempts", "border_attempts", "rounds", "n_reps"]
    assert C.sizeof(capi.GreedyStats) == sum(width[t] for t, _ in fields) == 40
    for (t, name), (_, ctype) in zip(fields, capi.GreedyStats._fields_):
        assert C.sizeof(ctype) == width[t], name
