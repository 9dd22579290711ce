"""rk_lca_rows on the device against tests/_lca_ref.py: the golden pairs under a star and a balanced binary taxonomy (cross-checked with
rk_group_sketches + rk_dist_rows), the three classes of list lengths at their seams (read from the call's stats, not copied), taxonomy
shapes, tiles and waves at their seams, the overflow of the partial records, multisets, 36-bit hashes, row shards, genome orders, the
host leg, the refusals, the empty cases and the tool.  Every case asserts from the stats which leg ran and what it counted, then
compares offsets, records, matched and unlabelled exactly."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _lca_ref as lr
from _selfjoin_cases import KMER, TOOL, device_index
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth
from test_gpu_gather import queries_of
from test_gpu_group import imported_index, index_of
from test_mask_cpu import golden

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
NONE = lr.NONE
ROWS_ARGTYPES = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.LcaStats)]


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def as_lists(parts):
    return [np.asarray(p).tolist() for p in parts]


def classified(ctx, idx, qs, refs, taxa, parent, queries, path=1, lists=None, attempts=1, **rows):
    """the call, with what every result must satisfy, compared exactly with the reference; returns (want rows, flat want, stats)"""
    off, recs, matched, unl, st = ctx.lca_rows(idx, qs, taxa, parent, **rows)
    refs, queries = as_lists(refs), as_lists(queries)
    lists = lists if lists is not None else lr.exported(refs)
    want = lr.from_lists(*lists, list(taxa), list(parent), queries)
    sel = lr.selected_rows(len(queries), rows.get("row_first", 0), rows.get("row_step", 1), rows.get("row_block", 0))
    w_off, w_recs, w_matched, w_unl = lr.flat(want, set(sel))
    total = sum(len(q) for q in queries)
    ran = bool(len(refs) and len(lists[0]) and sel)
    assert st["path"] == (path if ran else 0) and st["rows"] == len(sel) and st["elements"] == sum(len(queries[q]) for q in sel)
    assert off.tolist() == w_off and lr.records_of(recs) == w_recs
    assert [int(matched[q]) for q in sel] == [w_matched[q] for q in sel] and [int(unl[q]) for q in sel] == [w_unl[q] for q in sel]
    assert all(matched[q] == 0 and unl[q] == 0 for q in range(len(queries)) if q not in sel)   # (the binding's zeros: untouched)
    for r, m, u in (want[q] for q in sel):
        assert sum(d for _, d in r) + u == m
    assert st["matched"] == sum(w_matched[q] for q in sel) and st["unlabelled"] == sum(w_unl[q] for q in sel) and st["records"] == len(w_recs)
    if ran:
        lane, wave = st["lane_max"], st["wave_max"]
        assert 1 <= lane < wave < st["chunk"] and st["tile_hashes"] >= 64 and st["table_slots"] > st["tile_hashes"] and st["threads"] >= 64
        assert st["tiles"] == -(-total // st["tile_hashes"]) and st["lists"] == len(lists[0]) and st["postings"] == len(lists[1])
        assert st["lane_lists"] == sum(c <= lane for c in lists[2]) and st["wave_lists"] == sum(lane < c <= wave for c in lists[2])
        assert st["block_lists"] == sum(c > wave for c in lists[2]) and st["attempts"] == attempts
        if path == 1:
            assert st["records"] <= st["partials"] <= st["matched"]   # a record has a partial record; a partial record counts an element
        else:
            assert st["partials"] == 0 and st["longest_climb"] == 0
    return want, (w_off, w_recs, w_matched, w_unl), st


def constants(ctx):
    """the constants of the unit, from a first trivial call"""
    qs = queries_of(ctx, [np.array([1], dtype=np.uint32)])
    st = ctx.lca_rows(index_of(ctx, [np.array([1], dtype=np.uint32)]), qs, [0], [0])[4]
    assert st["path"] == 1 and st["tiles"] == 1 and st["matched"] == 1 and st["records"] == 1
    return st


def u32(x):
    return np.array(x, dtype=np.uint32)


def golden_counts(tag):
    """{(query name, reference name): common} of the real reference's `dist -D 1` on the golden pair: every pair has a line"""
    d, f = ("dist64", "dist64_M0_D1_N0.ref.txt") if tag == "64" else ("dist", "dist_M0_D1_N0.ref.txt")
    out = {}
    for line in open(os.path.join(GOLDEN, d, f)):
        q, r, counts = line.split("\t")[:3]
        out[(q, r)] = int(counts.split("|")[0])
    return out


def sketch_names(tag):
    d, s, read = ("dist64", "64", ok.read_sketches64) if tag == "64" else ("dist", "", ok.read_sketches32)
    return read(os.path.join(GOLDEN, d, "qry%s.sketch" % s))[1], read(os.path.join(GOLDEN, d, "ref%s.sketch" % s))[1]


# ---- 1. the golden pairs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,how", [("32", "built"), ("32", "imported"), ("64", "built"), ("64", "imported")])
def test_golden_pairs_under_a_star_and_a_binary_taxonomy(ctx, tag, how):
    ref, qry, _ = golden(tag)
    wide, bits = (True, 36) if tag == "64" else (False, 24)
    idx = (index_of if how == "built" else imported_index)(ctx, ref, wide, bits)
    qs = queries_of(ctx, qry, wide)
    lists = lr.exported(as_lists(ref))
    n = len(ref)
    want, _, st = classified(ctx, idx, qs, ref, list(range(1, n + 1)), lr.star(n), qry, lists=lists)
    assert st["matched"] > 0 and any(t == 0 for r, _, _ in want for t, _ in r) and any(t != 0 for r, _, _ in want for t, _ in r)
    parent, leaves = lr.balanced_binary(n)
    want, flat, st = classified(ctx, idx, qs, ref, leaves, parent, qry, lists=lists)
    assert st["longest_climb"] >= 1 and len(set(t for t, _ in flat[1])) > 3
    # the golden counts of the real reference: with reference v alone labelled, under a taxonomy of one node, the tally of a query is
    # the number of its hashes v holds -- the intersection count of the reference's own `dist` output (every pair is listed at -D 1)
    common = golden_counts(tag)
    q_names, r_names = sketch_names(tag)
    assert len(common) == len(qry) * n
    for v in (range(n) if how == "built" else range(0, n, 7)):
        off, recs, matched, unl, st = ctx.lca_rows(idx, qs, [0 if r == v else NONE for r in range(n)], [0])
        assert st["path"] == 1 and (matched - unl).tolist() == [common[(q, r_names[v])] for q in q_names]
        assert [d for _, d in lr.records_of(recs)] == [c for c in (common[(q, r_names[v])] for q in q_names) if c]
    # two oracles inside the project: clade(t) of a query = its common count with the markers (`only`) of the genomes under t
    called, clade = capi.lca_call(np.array(flat[1], dtype=capi.LCA_COUNT_DTYPE), flat[0], parent, (1, 0, 1, 0), clades=True)
    clade_of = [dict((t, int(c)) for (t, _), c in zip(flat[1][flat[0][q]:flat[0][q + 1]], clade[flat[0][q]:flat[0][q + 1]])) for q in range(len(qry))]
    seen = 0
    for t in range(len(parent)):
        under = [int(lr.is_ancestor(parent, t, leaf)) for leaf in leaves]
        sk, gl, gs, _ = ctx.group_sketches(idx, [0 if u else 1 for u in under], "markers")
        assert gl[0] == 0 and gs[0] == sum(under)
        dense = ctx.dist_rows(ctx.index_build(sk, bits), qs, 0, 0, KMER, 1.5, want_dense=True)[1]
        for q in range(len(qry)):
            below = sum(d for (tt, d) in want[q][0] if lr.is_ancestor(parent, t, tt))
            assert int(dense[q][0]) == below and clade_of[q].get(t, below) == below, (t, q)
            seen += below > 0
    assert seen > len(qry)
    for q in range(len(qry)):                                   # Kraken without confidence: the call is the candidate
        assert called[q]["taxon"] == called[q]["candidate"] and called[q]["retained"] == sum(d for _, d in want[q][0])


# ---- 2. the classes of list lengths ---------------------------------------------------------------------------------------------------------
def list_class_collection(st):
    """references, taxa and a query in which a list of every length around the seams occurs with the smallest and the largest preorder
    id at its first, a middle and its last posting, unlabelled postings at both ends, one taxon only, unlabelled holders only, and a
    reference that repeats the hash.  Taxonomy 0 -> (1 -> (4, 5), 2, 3): preorder 0 1 4 5 2 3, so 4 is the smallest and 2 the largest
    id in use."""
    parent = [0, 0, 0, 0, 1, 1]
    lengths = [st["lane_max"], st["lane_max"] + 1, st["wave_max"], st["wave_max"] + 1, st["chunk"], st["chunk"] + 1, 2 * st["chunk"] + 1]
    N = 2 * st["chunk"] + 9
    M = N // 2
    taxa = [5] * N
    for v, t in ((0, NONE), (1, 4), (2, 2), (M, 4), (M + 1, 2), (N - 3, 4), (N - 2, 2), (N - 1, NONE)):
        taxa[v] = t
    special = {0, 1, 2, M, M + 1, N - 3, N - 2, N - 1}
    plain = [v for v in range(N) if v not in special]
    variants = [({1, N - 2}, 0), ({2, N - 3}, 0), ({M, M + 1}, 0), ({1}, 1), ({N - 2}, 0), ({0, N - 1, M}, 1), (set(), 5), ({0, N - 1, 2}, 0)]
    refs = [[] for _ in range(N)]
    expect, h = {}, 100
    for L in lengths:
        for chosen, lca in variants:
            fill = [plain[int(i)] for i in np.linspace(0, len(plain) - 1, L - len(chosen)).round()]
            assert len(set(fill)) == len(fill) and len(fill) + len(chosen) == L
            for v in sorted(chosen | set(fill)):
                refs[v].append(h)
            expect[h] = (L, lca)
            h += 1
    for v in (0, N - 1):                       # unlabelled holders only
        refs[v].append(h)
    expect[h] = (2, NONE)
    h += 1
    for v in list(range(3, 3 + st["lane_max"])) + [3]:   # reference 3 repeats the hash: lane_max + 1 postings of lane_max genomes, all in 5
        refs[v].append(h)
    expect[h] = (st["lane_max"] + 1, 5)
    return parent, [u32(sorted(r)) for r in refs], taxa, expect


@pytest.mark.parametrize("how", ["built", "imported"])
def test_lists_of_every_class_at_the_seams(ctx, how):
    st = constants(ctx)
    parent, refs, taxa, expect = list_class_collection(st)
    idx = index_of(ctx, refs) if how == "built" else imported_index(ctx, refs, True, 36)
    wide = how != "built"
    dtype = np.uint64 if wide else np.uint32
    hashes = sorted(expect)
    queries = [np.array(hashes, dtype=dtype), np.array(hashes[::3] + hashes[::3] + [7], dtype=dtype)]
    lists = lr.exported(as_lists(refs))
    assert lists[2] == [expect[h][0] for h in hashes]
    want, _, got = classified(ctx, idx, queries_of(ctx, queries, wide), refs, taxa, parent, queries, lists=lists)
    tally = {}
    for h in hashes:
        tally[expect[h][1]] = tally.get(expect[h][1], 0) + 1
    assert want[0] == (sorted((t, d) for t, d in tally.items() if t != NONE), len(hashes), tally[NONE])   # the lcas worked out by hand
    assert got["lane_lists"] == 8 + 1 and got["wave_lists"] == 2 * 8 + 1 and got["block_lists"] == 4 * 8
    assert got["longest_climb"] == 2            # from 4 (or 5) over 1 to the root


# ---- 3. taxonomy shapes ---------------------------------------------------------------------------------------------------------------------
def test_a_taxonomy_of_one_node(ctx):
    refs = [u32([1, 2]), u32([2, 3]), u32([3, 4])]
    queries = [u32([1, 2, 3, 4, 5]), u32([4])]
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, [0, NONE, 0], [0], queries)
    assert want == [([(0, 4)], 4, 0), ([(0, 1)], 1, 0)] and st["longest_climb"] == 0
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, [NONE, NONE, 0], [0], queries)
    assert want == [([(0, 2)], 4, 2), ([(0, 1)], 1, 0)]


def test_a_path_of_300_nodes_is_climbed_once(ctx):
    """A path 0 - 1 - .. - 299 below the root 0 and one more leaf, 300, beside it: the deep end of the path has the smallest preorder id
    of a list held at 299 and at 300, and the climb from it to the root takes 299 parent steps.  (Holders at the two ends of the path
    alone climb 0 steps: the shallow end is the LCA and has the smallest preorder id.)"""
    parent = lr.path(300) + [0]
    refs = [u32([1, 2, 5]), u32([1, 3]), u32([2, 3, 4]), u32([4, 5])]
    taxa = [299, 300, 0, 150]
    queries = [u32([1, 2, 3, 4, 5, 6])]
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, taxa, parent, queries)
    assert want == [([(0, 4), (150, 1)], 5, 0)] and st["longest_climb"] == 299
    # both ends of the path alone
    want, _, st = classified(ctx, index_of(ctx, refs[:3:2]), queries_of(ctx, queries), refs[:3:2], [299, 0], parent, queries)
    assert want == [([(0, 3), (299, 2)], 5, 0)] and st["longest_climb"] == 0


def test_a_path_of_a_million_nodes_is_numbered_without_recursion(ctx, monkeypatch):
    """the preorder numbering of the device leg on a path of 10^6 nodes, worked by hand (the Python reference would walk the path per
    holder): A in the deep end, B in node 5, C in the root; hash 1: A, hash 2: A and B -> 5, hash 3: B and C -> 0"""
    T = 1_000_000
    parent = np.maximum(np.arange(T, dtype=np.int64) - 1, 0).astype(np.uint32)
    refs = [u32([1, 2]), u32([2, 3]), u32([3])]
    queries = [u32([1, 2, 3, 4]), u32([1, 1])]
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    for leg in (1, 2):
        if leg == 2:
            monkeypatch.setenv("RK_LCA_DEVICE", "0")
        off, recs, matched, unl, st = ctx.lca_rows(idx, qs, [T - 1, 5, 0], parent)
        assert st["path"] == leg and off.tolist() == [0, 3, 4] and lr.records_of(recs) == [(0, 1), (5, 1), (T - 1, 1), (T - 1, 2)]
        assert matched.tolist() == [3, 2] and unl.tolist() == [0, 0] and st["longest_climb"] == 0
    monkeypatch.delenv("RK_LCA_DEVICE")


def test_a_star_of_3000_leaves(ctx):
    n = 3000
    refs = [u32([7, 100 + v]) for v in range(n)]               # hash 7 is held by all: a list for a workgroup; the rest is private
    queries = [u32([7] + list(range(100, 100 + n))), u32([7, 7, 100, 3099, 5000])]
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, list(range(1, n + 1)), lr.star(n), queries)
    assert len(want[0][0]) == n + 1 and want[1] == ([(0, 2), (1, 1), (3000, 1)], 4, 0) and st["block_lists"] == 1 and st["longest_climb"] == 1


def test_a_caterpillar_and_five_renumberings_of_it(ctx):
    spine = 40
    parent = lr.caterpillar(spine)                              # no genome carries a spine node: every one of them is reached by an lca alone
    rng = np.random.default_rng(17)
    names, h, off = synth.clade_sketches(2 * spine, 50, 24, kmer_size=20, strains_per_clade=4, seed=3)
    refs = [h[int(off[v]):int(off[v + 1])] for v in range(2 * spine)]
    taxa = [NONE if v % 11 == 5 else spine + int(rng.integers(0, spine)) for v in range(2 * spine)]
    queries = [np.unique(np.concatenate([refs[int(m)] for m in rng.choice(2 * spine, size=3, replace=False)])) for _ in range(12)]
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    lists = lr.exported(as_lists(refs))
    want, _, st = classified(ctx, idx, qs, refs, taxa, parent, queries, lists=lists)
    assert any(t < spine for r, _, _ in want for t, _ in r) and st["unlabelled"] > 0 and st["longest_climb"] >= 2
    for k in range(5):
        perm = [int(x) for x in rng.permutation(len(parent))]
        parent2, taxa2 = lr.renumbered(parent, taxa, perm)
        again, _, _ = classified(ctx, idx, qs, refs, taxa2, parent2, queries, lists=lists)
        for (r, m, u), (r2, m2, u2) in zip(want, again):       # the results map onto each other
            assert sorted((perm[t], d) for t, d in r) == r2 and (m, u) == (m2, u2)


# ---- 4. tiles and waves -------------------------------------------------------------------------------------------------------------------------
SEAM_PARENT = [0, 0, 0, 1, 1]


def seam_refs(total):
    """four references over the hashes 0 .. total - 1: multiples of 2 (in node 3), of 3 (node 4), of 5 (node 2), of 7 (unlabelled)"""
    every = np.arange(total, dtype=np.uint32)
    return [every[every % 2 == 0], every[every % 3 == 0], every[every % 5 == 0], every[every % 7 == 0]], [3, 4, 2, NONE]


def runs(sizes):
    out, at = [], 0
    for s in sizes:
        out.append(np.arange(at, at + s, dtype=np.uint32))
        at += s
    return out


def seam_check(ctx, sizes, cache={}):
    total = sum(sizes)
    if total not in cache:
        refs, taxa = seam_refs(total)
        cache.clear()
        cache[total] = (refs, taxa, index_of(ctx, refs), lr.exported(as_lists(refs)))
    refs, taxa, idx, lists = cache[total]
    queries = runs(sizes)
    want, _, st = classified(ctx, idx, queries_of(ctx, queries), refs, taxa, SEAM_PARENT, queries, lists=lists)
    assert st["tiles"] == -(-total // st["tile_hashes"])
    return st


def test_totals_and_boundaries_around_a_tile_and_a_wave_seam(ctx):
    T = constants(ctx)["tile_hashes"]
    for total in (T - 1, T, T + 1, 2 * T + 1):
        seam_check(ctx, [total])
        seam_check(ctx, [total // 3, total - total // 3])
    for b in list(range(T - 2, T + 3)) + list(range(62, 67)) + list(range(T + 62, T + 67)) + [T - 64, T + 64]:
        seam_check(ctx, [b, 2 * T + 5 - b])
    seam_check(ctx, [T - 2, 1, 1, 1, 1, 62, 1, 1, 1, T - 61])   # a boundary at EVERY offset in [T - 2, T + 2] at once


def test_runs_of_empty_sketches(ctx):
    T = constants(ctx)["tile_hashes"]
    seam_check(ctx, [0, 0, 0, 5, 0, 0, T - 5, 0, 0, 0, 70, 0, 0])   # before, between (one run exactly on a tile boundary) and after
    seam_check(ctx, [0, T, 0, 0, T, 0])                             # the last offsets lie on the boundary behind the last tile
    refs, taxa = seam_refs(100)
    queries = [np.zeros(0, dtype=np.uint32)] * 3
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, taxa, SEAM_PARENT, queries)
    assert st["path"] == 1 and st["tiles"] == 0 and st["partials"] == 0 and want == [([], 0, 0)] * 3


def test_a_query_of_several_tiles_with_one_taxon(ctx):
    T = constants(ctx)["tile_hashes"]
    total = 3 * T + 17
    refs = [np.arange(total, dtype=np.uint32)]
    queries = [np.arange(total, dtype=np.uint32)]
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, [1], [0, 0], queries)
    assert want == [([(1, total)], total, 0)] and st["tiles"] == 4 and st["partials"] == st["tiles"] and st["records"] == 1


def test_a_tile_in_which_every_element_is_a_key_of_its_own(ctx):
    st = constants(ctx)
    n = st["tile_hashes"] + 150                                # a star of more leaves than a tile has elements, every leaf with a private hash
    refs = [u32([v]) for v in range(n)]
    taxa, parent = list(range(1, n + 1)), lr.star(n)
    idx = index_of(ctx, refs)
    queries = [np.arange(n, dtype=np.uint32)]                  # one row: the first tile holds tile_hashes different taxa, the table is full
    want, _, got = classified(ctx, idx, queries_of(ctx, queries), refs, taxa, parent, queries)
    assert got["partials"] == got["records"] == n and got["tiles"] == 2
    queries = [u32([v]) for v in range(n)]                     # more small queries than a tile has elements: every element is a row of its own
    want, _, got = classified(ctx, idx, queries_of(ctx, queries), refs, taxa, parent, queries)
    assert got["partials"] == got["records"] == n and want[n - 1] == ([(n, 1)], 1, 0)
    want, _, got = classified(ctx, idx, queries_of(ctx, queries), refs, [1] * n, [0, 0], queries)   # ... all in one taxon: the rows keep them apart
    assert got["partials"] == got["records"] == n


# ---- 5. the overflow of the partial records -------------------------------------------------------------------------------------------------
def test_partial_records_beyond_the_first_capacity_run_again(ctx, monkeypatch):
    T = constants(ctx)["tile_hashes"]
    refs, taxa = seam_refs(2 * T + 9)
    queries = runs([T - 3, 0, 40, T - 28])
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    want, flat, st = classified(ctx, idx, qs, refs, taxa, SEAM_PARENT, queries)
    assert st["attempts"] == 1 and st["partials"] > 4
    monkeypatch.setenv("RK_LCA_CAP", "1")
    again, flat2, st2 = classified(ctx, idx, qs, refs, taxa, SEAM_PARENT, queries, attempts=2)
    monkeypatch.setenv("RK_LCA_CAP", str(st["partials"]))      # exactly enough
    classified(ctx, idx, qs, refs, taxa, SEAM_PARENT, queries, attempts=1)
    monkeypatch.setenv("RK_LCA_CAP", str(st["partials"] - 1))  # one short
    classified(ctx, idx, qs, refs, taxa, SEAM_PARENT, queries, attempts=2)
    monkeypatch.delenv("RK_LCA_CAP")
    assert flat == flat2 and st2["partials"] == st["partials"]


# ---- 6. multisets -----------------------------------------------------------------------------------------------------------------------------
def test_a_query_that_repeats_hashes_counts_per_element(ctx):
    refs = [u32([9, 12]), u32([9, 9, 15]), u32([20])]          # the second reference repeats 9: a holder like any other
    taxa, parent = [1, 2, NONE], [0, 0, 0]
    queries = [u32([5, 5, 9, 9, 9, 12, 20, 20]), u32([15, 15, 15]), u32([3])]
    want, _, st = classified(ctx, index_of(ctx, refs), queries_of(ctx, queries), refs, taxa, parent, queries)
    assert want == [([(0, 3), (1, 1)], 6, 2), ([(2, 3)], 3, 0), ([], 0, 0)]


# ---- 7. hash widths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["built", "imported"])
def test_36_bit_hashes_and_hashes_beyond_them(ctx, how):
    bits = 36
    names, h, off = synth.clade_sketches(120, 60, bits, kmer_size=24, strains_per_clade=10, seed=29, wide=True)
    refs = [h[int(off[v]):int(off[v + 1])] for v in range(120)]
    parent = [0, 0, 0, 0] + [1 + c % 3 for c in range(12)]     # root, 3 groups, 12 clades of 10 strains
    # every other strain carries its clade, the rest the clade's group: what the strains of a clade share goes to the group
    taxa = [NONE if v % 17 == 3 else 4 + v // 10 if v % 2 == 0 else 1 + (v // 10) % 3 for v in range(120)]
    rng = np.random.default_rng(4)
    beyond = np.array([1 << bits, (1 << bits) + 5, (1 << 64) - 1], dtype=np.uint64)
    queries = [np.concatenate([np.unique(np.concatenate([refs[int(m)] for m in rng.choice(120, size=1 + k % 4, replace=False)])), beyond[:k % 4]])
               for k in range(20)]
    idx = (index_of if how == "built" else imported_index)(ctx, refs, True, bits)
    want, _, st = classified(ctx, idx, queries_of(ctx, queries, True), refs, taxa, parent, queries)
    assert st["matched"] == st["elements"] - sum(k % 4 for k in range(20)) and st["records"] >= 20 and any(0 < t < 4 for r, _, _ in want for t, _ in r)


# ---- 8. row shards ----------------------------------------------------------------------------------------------------------------------------
def test_row_shards_concatenate_and_leave_the_rest_alone(ctx):
    refs, taxa = seam_refs(700)
    queries = runs([60, 0, 100, 90, 1, 130, 200, 40, 79])
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    lists = lr.exported(as_lists(refs))
    want, whole, _ = classified(ctx, idx, qs, refs, taxa, SEAM_PARENT, queries, lists=lists)
    for block in (1, 2):
        matched, unl = np.full(len(queries), 0, dtype=np.uint32), np.full(len(queries), 0, dtype=np.uint32)
        recs = []
        for k in range(3):
            _, part, st = classified(ctx, idx, qs, refs, taxa, SEAM_PARENT, queries, lists=lists, row_first=k, row_step=3, row_block=block)
            assert st["rows"] == len(lr.selected_rows(len(queries), k, 3, block))
            off, r, m, u, _ = ctx.lca_rows(idx, qs, taxa, SEAM_PARENT, row_first=k, row_step=3, row_block=block, out=(matched, unl))   # one set of arrays
            recs.append((off, lr.records_of(r)))
        assert matched.tolist() == whole[2] and unl.tolist() == whole[3]
        joined = []
        for q in range(len(queries)):
            k = (q // block) % 3
            joined += recs[k][1][int(recs[k][0][q]):int(recs[k][0][q + 1])]
            assert all(recs[j][0][q] == recs[j][0][q + 1] for j in range(3) if j != k)
        assert joined == whole[1]


# ---- 9. genome order ----------------------------------------------------------------------------------------------------------------------------
def test_all_six_orders_of_a_three_clade_collection(ctx):
    names, h, off = synth.clade_sketches(30, 80, 24, kmer_size=20, strains_per_clade=10, seed=11)
    clades = [[h[int(off[v]):int(off[v + 1])] for v in range(10 * c, 10 * c + 10)] for c in range(3)]
    parent = [0, 0, 0, 1]                                       # clades 0 and 2 in the leaves 3 and 2, clade 1 in the inner node 1
    clade_taxon = [3, 1, 2]
    queries = [np.unique(np.concatenate([clades[0][1], clades[1][2]])), clades[2][0], np.unique(np.concatenate([clades[0][3], clades[2][4], u32([1, 2, 3])]))]
    qs = queries_of(ctx, queries)
    seen = []
    for order in itertools.permutations(range(3)):
        refs = [s for c in order for s in clades[c]]
        taxa = [clade_taxon[c] for c in order for _ in range(10)]
        want, flat, st = classified(ctx, index_of(ctx, refs), qs, refs, taxa, parent, queries)
        seen.append(flat)
    assert all(f == seen[0] for f in seen) and len(seen) == 6 and len(seen[0][1]) >= 4


# ---- 10. the host leg ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_the_host_leg_gives_the_same_arrays(ctx, wide, monkeypatch):
    ref, qry, _ = golden("64" if wide else "32")
    bits = 36 if wide else 24
    dtype = np.uint64 if wide else np.uint32
    queries = qry + [np.array([5, 5, 9], dtype=dtype), np.array([1 << bits, (1 << bits) + 1], dtype=dtype), ref[4]]   # (reference 4 is unlabelled)
    qs = queries_of(ctx, queries, wide)
    idx = index_of(ctx, ref, wide, bits)
    parent, leaves = lr.balanced_binary(len(ref))
    taxa = [NONE if v % 9 == 4 else leaves[v] for v in range(len(ref))]
    lists = lr.exported(as_lists(ref))
    for rows in ({}, {"row_first": 1, "row_step": 2, "row_block": 3}):
        device = ctx.lca_rows(idx, qs, taxa, parent, **rows)
        monkeypatch.setenv("RK_LCA_DEVICE", "0")
        want, _, st = classified(ctx, idx, qs, ref, taxa, parent, queries, path=2, lists=lists, **rows)
        host = ctx.lca_rows(idx, qs, taxa, parent, **rows)
        monkeypatch.delenv("RK_LCA_DEVICE")
        assert device[4]["path"] == 1 and host[4]["path"] == 2 and st["unlabelled"] > 0
        for d, h_ in zip(device[:4], host[:4]):
            assert d.tobytes() == h_.tobytes()
        for f in ("lists", "postings", "lane_lists", "wave_lists", "block_lists", "elements", "matched", "unlabelled", "records", "tiles", "rows"):
            assert device[4][f] == host[4][f], f


# ---- 11. what is refused ------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, qs, idx, taxa, parent, n_taxa=None, skip=None):
    L = capi.lib()
    L.rk_lca_rows.argtypes = ROWS_ARGTYPES
    q = qs.count if qs is not None else 1
    taxa, parent = u32(taxa), u32(parent)
    off = np.full(q + 1, 0x77, dtype=np.uint64)
    matched, unl = np.full(q, 0x77, dtype=np.uint32), np.full(q, 0x77, dtype=np.uint32)
    recs, n = C.c_void_p(0x1234), C.c_uint64(0x77)
    o, st = capi.LcaOpts(0, 0, 0), capi.LcaStats()
    args = [ctx._h, idx._h if idx is not None else None, qs._h if qs is not None else None, taxa.ctypes.data, parent.ctypes.data,
            len(parent) if n_taxa is None else n_taxa, C.byref(o), off.ctypes.data, C.byref(recs), C.byref(n), matched.ctypes.data, unl.ctypes.data, C.byref(st)]
    if skip is not None:
        args[skip] = None
    rc = L.rk_lca_rows(*args)
    untouched = recs.value == 0x1234 and n.value == 0x77 and (off == 0x77).all() and (matched == 0x77).all() and (unl == 0x77).all() and st.path == 0 and st.lists == 0
    return rc, untouched


def test_arguments_that_are_refused(ctx):
    refs = [u32([1, 2]), u32([2, 3])]
    queries = [u32([1, 2, 3]), u32([9])]
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    good = ([1, NONE], [0, 0])
    for skip in (1, 2, 3, 4, 6, 7, 8, 9, 10, 11):       # idx, queries, taxa, parent, opts, off, counts, n_counts, matched, unlabelled
        assert raw_call(ctx, qs, idx, *good, skip=skip) == (RK_ERR_ARG, True), skip
    assert raw_call(ctx, qs, idx, *good, n_taxa=0) == (RK_ERR_ARG, True)
    for parent in ([0, 1], [1, 0], [0, 2], [0, 2, 1], [1, 2, 0, 3]):     # two roots, none, a parent beyond the nodes, a cycle beside the root, both
        assert raw_call(ctx, qs, idx, [0, NONE], parent) == (RK_ERR_ARG, True) and b"root" in last(), parent
    assert raw_call(ctx, qs, idx, [2, NONE], [0, 0]) == (RK_ERR_ARG, True) and b"taxon" in last()
    assert raw_call(ctx, qs, idx, [0x80000000, NONE], [0, 0]) == (RK_ERR_ARG, True)
    assert raw_call(ctx, qs, idx, *good, n_taxa=2 ** 31) == (RK_ERR_UNSUPPORTED, True)
    wide = index_of(ctx, [np.array([1 << 33], dtype=np.uint64)] * 2, True, 36)
    assert raw_call(ctx, qs, wide, *good) == (RK_ERR_ARG, True) and b"widths" in last()
    assert raw_call(ctx, queries_of(ctx, [np.array([1 << 33], dtype=np.uint64)], True), idx, *good) == (RK_ERR_ARG, True) and b"widths" in last()
    with pytest.raises(capi.RkError) as e:
        ctx.lca_rows(idx, qs, [1, NONE], [1, 0])
    assert e.value.code == RK_ERR_ARG
    with pytest.raises(ValueError):
        ctx.lca_rows(idx, qs, [1], [0, 0])
    assert raw_call(ctx, qs, idx, *good, skip=12)[0] == 0                                   # the stats are optional


def test_indexes_without_all_posting_lists_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    qs = queries_of(ctx, [h[int(off[v]):int(off[v + 1])] for v in range(3)])
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    assert raw_call(ctx, qs, parts[0], [0] * 1600, [0]) == (RK_ERR_ARG, True)   # one hash range of a sharded build
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    recv = torch.cat([bufs[r][: 12 * sent[r][0]] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
    torch.cuda.synchronize()
    j = ctx.index_join_shard(parts[0], recv.data_ptr(), sum(sent[r][0] for r in range(S)))
    capi.lib().rk_lca_rows.argtypes = ROWS_ARGTYPES
    assert raw_call(ctx, qs, j, [0] * 1600, [0]) == (RK_ERR_ARG, True)   # the join-only index: tile records of its rows, no lists
    assert b"posting lists" in capi.lib().rk_last_error(ctx._h)
    del j, parts, sk


# ---- 12. the empty cases ------------------------------------------------------------------------------------------------------------------------
def test_no_query_no_genome_no_labelled_genome(ctx):
    refs = [u32([1, 2]), u32([2, 3])]
    queries = [u32([1, 2, 3, 4]), u32([]), u32([2, 2])]
    idx, qs = index_of(ctx, refs), queries_of(ctx, queries)
    none_q = ctx.sketches_from_host(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))
    off, recs, matched, unl, st = ctx.lca_rows(idx, none_q, [0, 0], [0])
    assert off.tolist() == [0] and len(recs) == len(matched) == len(unl) == 0 and st["path"] == 0 and st["tiles"] == st["tile_hashes"] == 0
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 24)
    assert none.genomes == 0
    want, _, st = classified(ctx, none, qs, [], [], [0, 0], queries)
    assert want == [([], 0, 0)] * 3 and st["path"] == 0
    empty = index_of(ctx, [u32([]), u32([])])                   # genomes without hashes
    want, _, st = classified(ctx, empty, qs, [[], []], [0, 1], [0, 0], queries)
    assert want == [([], 0, 0)] * 3 and st["path"] == 0
    want, _, st = classified(ctx, idx, qs, refs, [NONE, NONE], [0, 0], queries)   # no labelled genome: matched is still counted
    assert want == [([], 3, 3), ([], 0, 0), ([], 2, 2)] and st["path"] == 1 and st["records"] == 0 and st["partials"] == 2


# ---- 13. the tool -------------------------------------------------------------------------------------------------------------------------------
def run_tool(cwd, args):
    return subprocess.run([TOOL] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def golden_files(tag, tmp_path):
    d, s = ("dist64", "64") if tag == "64" else ("dist", "")
    shutil.copy(os.path.join(GOLDEN, d, "ref%s.sketch" % s), tmp_path / "ref.sketch")
    shutil.copy(os.path.join(GOLDEN, d, "qry%s.sketch" % s), tmp_path / "qry.sketch")
    for f in ("taxonomy.tsv", "taxa%s.txt" % s):
        shutil.copy(os.path.join(GOLDEN, "lca", f), tmp_path / f)
    read = ok.read_sketches64 if tag == "64" else ok.read_sketches32
    return read(str(tmp_path / "qry.sketch"))[1], "taxa%s.txt" % s


def parsed_taxonomy(tmp_path, taxa_file):
    rows = [line.rstrip("\n").split("\t") for line in open(tmp_path / "taxonomy.tsv") if line.strip()]
    ids = sorted(int(r[0]) for r in rows)
    node = {x: k for k, x in enumerate(ids)}
    parent, name = [0] * len(ids), [""] * len(ids)
    for r in rows:
        parent[node[int(r[0])]] = node[int(r[1])]
        name[node[int(r[0])]] = r[2] if len(r) > 2 else ""
    taxa = [NONE if line.strip() == "-" else node[int(line)] for line in open(tmp_path / taxa_file)]
    return ids, parent, name, taxa


def tool_text(names, queries, want, ids, parent, name, rule):
    out, summary = [], []
    for q, (recs, matched, unl) in enumerate(want):
        c, clade = lr.call(recs, parent, rule, len(queries[q]))
        called = "-\t-" if c["taxon"] == NONE else "%d\t%s" % (ids[c["taxon"]], name[c["taxon"]])
        cand = "-" if c["candidate"] == NONE else "%d" % ids[c["candidate"]]
        out.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (names[q], called, cand, c["clade"], c["retained"], matched, unl, len(queries[q])))
        summary += ["%s\t%d\t%s\t%d\t%d\n" % (names[q], ids[t], name[t], d, cl) for (t, d), cl in zip(recs, clade)]
    return "".join(out).encode(), "".join(summary).encode()


@pytest.mark.parametrize("tag", ["32", "64"])
def test_tool_lca_writes_the_calls_and_the_summary(ctx, tag, tmp_path):
    ref, qry, _ = golden(tag)
    names, taxa_file = golden_files(tag, tmp_path)
    ids, parent, name, taxa = parsed_taxonomy(tmp_path, taxa_file)
    assert len(taxa) == len(ref) and NONE in taxa and lr.is_taxonomy(parent)
    want = lr.from_lists(*lr.exported(as_lists(ref)), taxa, parent, as_lists(qry))
    base = ["lca", "-r", "ref.sketch", "-q", "qry.sketch", "--taxonomy", "taxonomy.tsv", "--taxa", taxa_file]
    texts = set()
    for args, rule in (([], (1, 0, 1, 0)), (["--min-count", "3", "--confidence", "1/1"], (3, 1, 1, 0)), (["--confidence", "1/2", "--of", "sketch"], (1, 1, 2, 1)),
                       (["--confidence", "2/3", "--of", "labelled"], (1, 2, 3, 0)), (["--min-count", "250"], (250, 0, 1, 0))):
        p = run_tool(tmp_path, base + ["-o", "out.txt", "--summary", "sum.txt"] + args)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        w_out, w_sum = tool_text(names, qry, want, ids, parent, name, rule)
        assert (tmp_path / "out.txt").read_bytes() == w_out and (tmp_path / "sum.txt").read_bytes() == w_sum, args
        texts.add(w_out)
    assert len(texts) >= 3 and len(w_sum.splitlines()) > len(qry)


def test_tool_lca_dies_on_bad_input(ctx, tmp_path):
    names, taxa_file = golden_files("32", tmp_path)
    good_tax = (tmp_path / "taxonomy.tsv").read_text()
    good_taxa = (tmp_path / taxa_file).read_text()
    base = ["lca", "-r", "ref.sketch", "-q", "qry.sketch", "--taxonomy", "t.tsv", "--taxa", "x.txt", "-o", "x.out"]
    first = good_tax.splitlines()[0]
    cases = [(good_tax + first + "\n", good_taxa, [], b"twice"),
             (good_tax + "777\t778\torphan\n", good_taxa, [], b"is no node of"),
             (good_tax + "777\t777\tanother root\n", good_taxa, [], b"2 roots"),
             ("5\t6\ta\n6\t5\tb\n", "-\n" * good_taxa.count("\n"), [], b"0 roots"),
             (good_tax + "x\t1\n", good_taxa, [], b"not id<TAB>parent id"),
             (good_tax + " 7\t1\n", good_taxa, [], b"not id<TAB>parent id"),
             (good_tax + "99999999999999999999\t1\n", good_taxa, [], b"not id<TAB>parent id"),
             (good_tax, good_taxa + "-\n", [], b"holds more than"),
             (good_tax, good_taxa.split("\n", 1)[1], [], b"lines, the input"),
             (good_tax, "424242\n" + good_taxa.split("\n", 1)[1], [], b"neither an id of the taxonomy nor -"),
             (good_tax, good_taxa, ["--min-count", "0"], b"--min-count needs an integer"),
             (good_tax, good_taxa, ["--confidence", "3/2"], b"--confidence needs P/Q"),
             (good_tax, good_taxa, ["--confidence", "0.5"], b"--confidence needs P/Q"),
             (good_tax, good_taxa, ["--of", "all"], b"--of must be labelled or sketch"),
             (good_tax, good_taxa, ["--gpus", "2"], b"one GPU")]
    for tax, taxa, args, text in cases:
        (tmp_path / "t.tsv").write_text(tax)
        (tmp_path / "x.txt").write_text(taxa)
        p = run_tool(tmp_path, base + args)
        assert p.returncode != 0 and text in p.stderr and not (tmp_path / "x.out").exists(), (args, text, p.stderr[-300:])
    p = run_tool(tmp_path, ["lca", "-r", "ref.sketch", "-q", "qry.sketch", "-o", "x.out"])
    assert p.returncode != 0 and b"lca needs -r, -q, --taxonomy, --taxa and -o" in p.stderr
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"lca     -r" in p.stderr and b" merge lca info " in p.stderr and b"--taxonomy FILE" in p.stderr
