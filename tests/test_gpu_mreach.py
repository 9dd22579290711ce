"""rk_mreach_rows: the minimum spanning forest of the self join under mutual-reachability distance against tests/_mreach_ref.py (exact
rational ratios, sorted adjacencies, a Kruskal) over the ORACLE's hit list, set up from tests/_selfjoin_cases.py (its Oracle, device_index
and collections, built once per session): core distances, core neighbours and edges, exactly, jorc and dist bit for bit.  Every case says
from the call's stats that it reached the edge it is about."""
import ctypes as C
import itertools
import math
import subprocess

import numpy as np
import pytest

import _dbscan_ref as dr
import _mreach_ref as mr
from _selfjoin_cases import (KMER, TOOL, Oracle, both_overflows_collection, both_overflows_thresholds, collection, csr, device_index,
                             identical, permuted, tie_collection)
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def check(got, hits, n, min_pts, metric):
    """(core_dist, core_nb, edges, stats) of one call against the reference over the oracle's hit list `hits`; returns the reference's
    (core, edges)"""
    core_dist, core_nb, edges, st = got
    tuples = mr.hit_tuples(hits)
    core, want = mr.mreach(tuples, n, min_pts, metric)
    at = {t[:2]: i for i, t in enumerate(tuples)}
    assert core_dist.dtype == np.float64 and core_nb.dtype == np.uint32 and edges.dtype == capi.HIT_DTYPE
    assert core_nb.tolist() == [mr.NONE if c is None else c[1] for c in core]
    assert core_dist.tolist() == [0.0 if min_pts == 1 else INF if c is None else float(hits["dist"][at[c[0][:2]]]) for c in core]   # bit for bit
    assert mr.hit_tuples(edges) == want
    where = np.array([at[e[:2]] for e in want], dtype=np.int64)
    assert np.array_equal(edges["jorc"], hits["jorc"][where]) and np.array_equal(edges["dist"], hits["dist"][where])
    assert st["n_trees"] == n - len(want) and st["n_core"] == (n if min_pts == 1 else sum(c is not None for c in core))
    if st["path"] == 1:
        assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
        assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(hits)   # the device consumed exactly the oracle's pairs
        limit = 2 + max(0, math.ceil(math.log2(n)))
        assert st["rounds"] <= limit and (st["rounds"] >= 1) == (len(hits) > 0)
    else:
        assert st["path"] == 2 and st["edges"] == len(hits) and st["join_attempts"] == 0 and st["rounds"] == 0
    return core, want


def degrees(hits, n):
    return np.bincount(np.concatenate([hits["row"], hits["col"]]).astype(np.int64), minlength=n)


# ---- 1. the comparator: every pair at distance 0 ------------------------------------------------------------------------
def test_identical_sketches_give_the_star_of_genome_0_or_nothing(ctx):
    h, off = csr(permuted(identical(300, 2), 12))
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 300 * 299 // 2 and np.all(hits["dist"] == 0.0)
    idx = device_index(ctx, h, off, 24)
    for min_pts, path in ((5, 1), (65, 1), (66, 2)):   # every weight is equal: (row, col) decides everything; k = 64 is the last on the device
        got = ctx.mreach_rows(idx, 0, KMER, 0.05, min_pts)
        check(got, hits, 300, min_pts, 0)
        core_dist, core_nb, edges, st = got
        assert st["path"] == path and st["n_trees"] == 1 and st["n_core"] == 300 and not core_dist.any()
        assert edges["row"].tolist() == [0] * 299 and edges["col"].tolist() == list(range(1, 300))
        k = min_pts - 1
        assert core_nb.tolist() == [k if v < k else k - 1 for v in range(300)]   # the k-th smallest index that is not v
        if path == 1:
            assert st["max_degree"] == 299 and st["edges"] == 44850 and st["rounds"] >= 2
    got = ctx.mreach_rows(idx, 0, KMER, 0.05, 301)   # deg + 1 < min_pts everywhere
    check(got, hits, 300, 301, 0)
    assert len(got[2]) == 0 and np.all(np.isinf(got[0])) and np.all(got[1] == mr.NONE) and got[3]["n_trees"] == 300 and got[3]["n_core"] == 0


# ---- 2. degrees at the seam between two chunks of the selection wave ----------------------------------------------------
_cliques = {}


def cliques():
    """cliques of 64, 65, 66 and 129 sketches (degrees 63, 64, 65 and 128): 100 hashes each, 80 .. 95 of them from the clique's 100 (any
    two share 60 or more: d <= 0.026), in a fixed random caller order"""
    if not _cliques:
        rng = np.random.default_rng(43)
        pool = np.unique(rng.integers(0, 1 << 24, size=12000))
        rng.shuffle(pool)
        parts, used = [], 0
        for size in (64, 65, 66, 129):
            base = pool[used: used + 100]
            used += 100
            for _ in range(size):
                share = int(rng.integers(80, 96))
                parts.append(np.sort(np.concatenate([rng.choice(base, size=share, replace=False), pool[used: used + 100 - share]])))
                used += 100 - share
        h, off = csr(permuted(parts, 44))
        _cliques["it"] = (h, off, Oracle(h, off, 24))
    return _cliques["it"]


@pytest.mark.parametrize("k", [1, 63, 64])
def test_degrees_at_the_chunk_seam(ctx, k):
    h, off, orc = cliques()
    n = len(off) - 1
    hits = orc.hits(0, 0.05)
    deg = degrees(hits, n)
    assert sorted(set(deg.tolist())) == [63, 64, 65, 128] and len(hits) == (64 * 63 + 65 * 64 + 66 * 65 + 129 * 128) // 2
    assert len(set(hits["common"].tolist())) > 20   # random shares: many ratios
    got = ctx.mreach_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, k + 1)
    core, edges = check(got, hits, n, k + 1, 0)
    st = got[3]
    assert st["path"] == 1 and st["max_degree"] == 128 and st["join_attempts"] == 1
    bare = [v for v in range(n) if core[v] is None]
    assert bare == ([] if k < 64 else np.flatnonzero(deg == 63).tolist())   # degree 63 at k = 64: no core record, no edge
    assert st["n_trees"] == (4 if k < 64 else 3 + 64) and len(edges) == n - st["n_trees"]


# ---- 3. chaining: a genome between two groups ---------------------------------------------------------------------------
def chain_parts(seed, equal):
    """([A, B, x], the rest): two groups of three identical sketches A and B that share nothing, their satellites (five per group, each
    with the part of its group's sketch that x does not touch: adjacent to the group and to each other, never to x), and x, which holds
    hashes of both groups' sketches.  The rest: the other two copies of A and of B, then the satellites.
    equal: |A| = 35, |B| = 55, |x| = 45 with 20 of A and 25 of B -- jaccard 20/60 = 25/75, d = 0.0347 both; satellites at 15/40 and 30/65.
    else : 100 hashes each, x with 40 of A (40/160, d = 0.0458) and 30 of B (30/170, d = 0.0602); satellites at 60/140.
    deg(x) = 6, deg(a copy) = 2 + 1 + 5 = 8, deg(a satellite) = 3 + 4 = 7."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 24, size=2000))
    rng.shuffle(pool)
    used = [0]

    def fresh(k):
        used[0] += k
        return pool[used[0] - k: used[0]]
    if equal:
        A, B = fresh(35), fresh(55)
        x = np.concatenate([A[:20], B[:25]])
        sat = [np.concatenate([A[20:], fresh(5)]) for _ in range(5)] + [np.concatenate([B[25:], fresh(10)]) for _ in range(5)]
    else:
        A, B = fresh(100), fresh(100)
        x = np.concatenate([A[:40], B[:30], fresh(30)])
        sat = [np.concatenate([A[40:], fresh(40)]) for _ in range(5)] + [np.concatenate([B[30:], fresh(40)]) for _ in range(5)]
    return [np.sort(p) for p in (A, B, x)], [np.sort(p) for p in [A, A, B, B] + sat]


def x_edges_by_the_tie_break(hits, x, a_copies):
    """what (row, col) picks among x's six hits when all of them weigh the same: the first of them, then the first into the other group"""
    mine = sorted(t[:2] for t in mr.hit_tuples(hits) if x in t[:2])
    assert len(mine) == 6
    side = [(p[0] + p[1] - x) in a_copies for p in mine]
    return [mine[0], mine[side.index(not side[0])]]


def test_a_genome_between_two_groups_is_isolated_or_ties_on_its_core_distance(ctx):
    first, rest = chain_parts(7, equal=False)
    order = np.random.default_rng(8).permutation(3 + len(rest))
    parts = first + rest
    h, off = csr([parts[i] for i in order])
    n = len(parts)
    where = {int(src): at for at, src in enumerate(order)}
    x, a_copies = where[2], sorted(where[i] for i in (0, 3, 4))
    hits = Oracle(h, off, 24).hits(0, 0.07)
    assert degrees(hits, n)[x] == 6
    idx = device_index(ctx, h, off, 24)
    forest, fst = ctx.forest_rows(idx, 0, KMER, 0.07)
    assert fst["n_trees"] == 1   # single linkage chains the two groups through x
    got = ctx.mreach_rows(idx, 0, KMER, 0.07, 8)   # k = 7 > deg(x): x has no core record
    core, edges = check(got, hits, n, 8, 0)
    assert core[x] is None and got[0][x] == INF and all(x not in e[:2] for e in edges)
    assert got[3]["n_trees"] == 3 and got[3]["n_core"] == n - 1 and got[3]["path"] == 1   # the two groups, and x alone
    got = ctx.mreach_rows(idx, 0, KMER, 0.07, 7)   # k = 6 = deg(x): its farthest pair weighs on all six
    core, edges = check(got, hits, n, 7, 0)
    far = max(float(d) for t, d in zip(mr.hit_tuples(hits), hits["dist"]) if x in t[:2])
    assert got[0][x] == far and got[3]["n_trees"] == 1
    mine = [e for e in edges if x in e[:2]]
    assert [e[:2] for e in mine] == x_edges_by_the_tie_break(hits, x, a_copies) and mine == edges[-2:]   # the heaviest, and (row, col) among them
    assert all(max(float(e["dist"]), got[0][e["row"]], got[0][e["col"]]) == far for e in got[2][-2:])


@pytest.mark.parametrize("roles", list(itertools.permutations(range(3))))
def test_equal_ratio_from_different_counts_ties_under_every_index_order(ctx, roles):
    first, rest = chain_parts(9, equal=True)
    h, off = csr([first[r] for r in roles] + rest)   # the first copy of A, the first of B and x at the caller indices 0, 1, 2 in every order
    n = 3 + len(rest)
    a, b, x = roles.index(0), roles.index(1), roles.index(2)
    hits = Oracle(h, off, 24).hits(0, 0.07)
    tuples = {t[:2]: t for t in mr.hit_tuples(hits)}
    ta, tb = tuples[(min(a, x), max(a, x))], tuples[(min(b, x), max(b, x))]
    assert (ta[2], tb[2]) == (20, 25) and ta[2] * (tb[3] + tb[4] - tb[2]) == tb[2] * (ta[3] + ta[4] - ta[2])   # 20/60 == 25/75
    idx = device_index(ctx, h, off, 24)
    for min_pts in (7, 2):   # x's six pairs tie with its core distance, and with each other without it
        got = ctx.mreach_rows(idx, 0, KMER, 0.07, min_pts)
        core, edges = check(got, hits, n, min_pts, 0)
        assert got[3]["n_trees"] == 1 and got[3]["path"] == 1
        assert [e[:2] for e in edges if x in e[:2]] == x_edges_by_the_tie_break(hits, x, [a, 3, 4])
    assert core[x][1] == min(a, b, 3)   # (min_pts 2) the nearest of six equals: the smallest index


# ---- 4. one ratio from different counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_tie_collection(ctx, metric):
    h, off = tie_collection(3)   # six triangles at 25/75 = 20/60 = 20/60, one per assignment of the roles to ascending indices, and six plain pairs
    n = len(off) - 1
    hits = Oracle(h, off, 24).hits(metric, 0.06)
    idx = device_index(ctx, h, off, 24)
    for min_pts in (1, 2, 3, 4):
        got = ctx.mreach_rows(idx, metric, KMER, 0.06, min_pts)
        core, edges = check(got, hits, n, min_pts, metric)
        if metric == 0 and min_pts <= 3:   # a triangle's three pairs weigh the same: its forest is its two smallest pairs
            tri = [e[:2] for e in edges if e[2] in (20, 25)]
            assert len(tri) == 12 and all(p[0] % 5 == 0 or p == (p[0], p[0] + 1) for p in tri) and any(e[2] == 20 for e in edges) and any(e[2] == 25 for e in edges)
    assert len(edges) == 0 and got[3]["n_core"] == 0   # (min_pts 4: no genome has three pairs)


# ---- 5. union-find depth and the number of rounds: a path ---------------------------------------------------------------
@pytest.mark.parametrize("order", ["identity", "permuted"])
def test_path_of_2048_genomes(ctx, order):
    # a window of 100 hashes that moves on by 5, 6 or 7: neighbours share 93 .. 95 (d <= 0.00363), next but one 86 .. 90 (d >= 0.00527)
    n, m = 2048, 100
    rng = np.random.default_rng(1)
    start = np.concatenate([[0], np.cumsum(rng.integers(5, 8, size=n - 1))])
    pool = np.unique(rng.integers(0, 1 << 24, size=int(start[-1]) + m + 4000))[: int(start[-1]) + m]
    assert len(pool) == int(start[-1]) + m
    parts = [pool[s: s + m] for s in start.tolist()]
    at = list(range(n))
    if order == "permuted":
        perm = np.random.default_rng(11).permutation(n)
        parts = [parts[i] for i in perm]
        at = np.argsort(perm).tolist()   # at[i]: the caller index of the path's i-th genome
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.0045)
    assert len(hits) == n - 1 and len(set(hits["common"].tolist())) == 3
    got = ctx.mreach_rows(device_index(ctx, h, off, 24), 0, KMER, 0.0045, 3)
    core, edges = check(got, hits, n, 3, 0)
    core_dist, core_nb, _, st = got
    assert st["path"] == 1 and st["max_degree"] == 2 and st["join_attempts"] == 1 and st["border_attempts"] == 1
    assert 3 <= st["rounds"] <= 2 + 11   # 2 + ceil(log2 2048)
    assert sorted(np.flatnonzero(np.isinf(core_dist)).tolist()) == sorted([at[0], at[n - 1]]) and st["n_core"] == n - 2   # the ends
    assert len(edges) == n - 3 and st["n_trees"] == 3   # the interior in one tree, the two ends alone
    d = {(int(r), int(c)): float(x) for r, c, x in zip(hits["row"], hits["col"], hits["dist"])}
    for i in range(1, n - 1):   # the farther of two neighbours
        pair = [d[(min(at[i], at[j]), max(at[i], at[j]))] for j in (i - 1, i + 1)]
        assert core_dist[at[i]] == max(pair)


# ---- 6. contention: a star ----------------------------------------------------------------------------------------------
def test_star_of_3000_leaves(ctx):
    rng = np.random.default_rng(2)   # the star of the kNN suite
    pool = np.unique(rng.integers(0, 1 << 24, size=140000))
    rng.shuffle(pool)
    hub, spare = pool[:100], pool[100:]
    parts = [np.sort(hub)]
    for j in range(3000):   # a leaf: 60 of the hub's hashes and 40 of its own -- hub-leaf d = 0.0255, leaf-leaf ~0.05
        parts.append(np.sort(np.concatenate([rng.choice(hub, size=60, replace=False), spare[40 * j: 40 * j + 40]])))
    order = np.random.default_rng(12).permutation(3001)
    h, off = csr([parts[i] for i in order])
    centre = int(np.flatnonzero(order == 0)[0])
    idx = device_index(ctx, h, off, 24)
    hits = Oracle(h, off, 24).hits(0, 0.03)
    assert len(hits) == 3000 and np.all((hits["row"] == centre) | (hits["col"] == centre))   # the star alone: no two leaves within -D
    got = ctx.mreach_rows(idx, 0, KMER, 0.03, 2)   # the hub's segment streams in 47 chunks of 64
    check(got, hits, 3001, 2, 0)
    core_dist, core_nb, edges, st = got
    leaves = np.arange(3001) != centre
    assert st["path"] == 1 and st["max_degree"] == 3000 and len(edges) == 3000 and st["n_trees"] == 1 and st["n_core"] == 3001
    assert np.all(core_nb[leaves] == centre) and core_nb[centre] == (1 if centre == 0 else 0)   # every pair at 60/140: the smallest index
    got = ctx.mreach_rows(idx, 0, KMER, 0.03, 3)   # a leaf has one pair: no core record, and no edge without the leaves
    check(got, hits, 3001, 3, 0)
    assert len(got[2]) == 0 and got[3]["n_core"] == 1 and got[3]["n_trees"] == 3001 and got[0][centre] < INF and np.all(np.isinf(got[0][leaves]))


# ---- 7. borderline records decide core records, behind both overflows ---------------------------------------------------
def test_borderline_records_decide_core_records_behind_both_overflows(ctx, monkeypatch):
    h, off = both_overflows_collection()
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    for D, n_hits, kept in both_overflows_thresholds():
        hits = orc.hits(0, D)
        assert len(hits) == n_hits > 65536
        got = ctx.mreach_rows(idx, 0, KMER, D, 2)
        check(got, hits, 420, 2, 0)
        core_dist, core_nb, edges, st = got
        assert st["path"] == 1 and st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        # one ulp above: the ten pairs are linked, with finite core distances; on the distance itself: twenty genomes without a core record
        assert (len(edges), st["n_core"], st["n_trees"]) == ((399 + 10, 420, 11) if kept else (399, 400, 21))
        assert int(np.isinf(core_dist).sum()) == (0 if kept else 20) and int((edges["common"] == 80).sum()) == kept


# ---- 8. a borderline edge that gives a genome its k-th neighbour --------------------------------------------------------
def cascade_collection():
    """Two clusters P and Q, each a sketch P0 / Q0 of 100 hashes and three copies of a sketch that holds 65 of its hashes; g holds the
    other 35 of P0, the other 35 of Q0 and 30 of its own (g - P0 and g - Q0 at 35/165, d = 0.0525), z those 30 and 70 of its own (z - g
    at 30/170, d = -ln(0.3) / 20 = 0.0602).  deg(g) = 2 without z: at min_pts 4 the edge z - g is g's third, gives g a core record, and
    with it g's two other pairs a finite weight: P0 and Q0 then hang in ONE tree.  Returns (h, off, g, z, p0, q0) in a fixed random
    caller order."""
    rng = np.random.default_rng(25)
    pool = np.unique(rng.integers(0, 1 << 24, size=1000))
    rng.shuffle(pool)
    P0, Q0, own, zown, pown, qown = pool[:100], pool[100:200], pool[200:230], pool[230:300], pool[300:335], pool[335:370]
    g = np.concatenate([P0[:35], Q0[:35], own])
    z = np.concatenate([own, zown])
    P1, Q1 = np.concatenate([P0[35:], pown]), np.concatenate([Q0[35:], qown])
    parts = [np.sort(p) for p in (g, z, P0, Q0, P1, P1, P1, Q1, Q1, Q1)]
    order = np.random.default_rng(26).permutation(len(parts))
    h, off = csr([parts[i] for i in order])
    where = [int(np.flatnonzero(order == i)[0]) for i in range(4)]
    return (h, off) + tuple(where)


@pytest.mark.parametrize("metric", [0, 1])
def test_borderline_edge_gives_a_genome_its_core_record_and_joins_two_trees(ctx, metric):
    h, off, g, z, p0, q0 = cascade_collection()
    n = len(off) - 1
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    for D, joined in ((float(np.nextafter(d0, 0.0)), False), (d0, False), (float(np.nextafter(d0, 1.0)), True)):   # strict <
        hits = orc.hits(metric, D)
        assert ((min(g, z), max(g, z)) in {t[:2] for t in mr.hit_tuples(hits)}) == joined   # where the oracle's hit list flips
        got = ctx.mreach_rows(idx, metric, KMER, D, 4)
        core, edges = check(got, hits, n, 4, metric)
        core_dist, core_nb, _, st = got
        assert st["path"] == 1 and st["borderline"] >= 1 and st["borderline_kept"] == int(joined)
        labels = capi.mreach_cut(got[2], core_dist, D)
        if joined:   # z - g is g's third pair and its core record; z itself has one pair: no core record, no edge
            assert core_nb[g] == z and core_dist[g] == d0 and core_dist[z] == INF and st["n_trees"] == 2 and st["n_core"] == n - 1
            assert labels[p0] == labels[q0] == labels[g] != dr.NOISE and labels[z] == dr.NOISE
            assert sum(g in e[:2] for e in edges) == 2 and all(z not in e[:2] for e in edges)
        else:        # g has two pairs: it hangs nowhere, and P0 and Q0 in two trees
            assert core_dist[g] == INF and core_dist[z] == INF and st["n_trees"] == 4 and st["n_core"] == n - 2
            assert dr.NOISE != labels[p0] != labels[q0] != dr.NOISE and labels[g] == labels[z] == dr.NOISE


# ---- 9. every kernel of the join, both metrics, 36-bit hashes -----------------------------------------------------------
@pytest.mark.parametrize("which,kernel,metric", [
    ("tiles", "rk_tile_kernel", 0), ("tiles", "rk_tile_kernel", 1), ("near", "rk_near_kernel", 0), ("near", "rk_near_kernel", 1),
    ("repeat", "rk_dist_kernel", 0), ("repeat", "rk_dist_kernel", 1), ("wide", None, 0), ("wide", None, 1)])
def test_every_join_kernel_both_metrics_and_wide_hashes(ctx, which, kernel, metric):
    # ("repeat": one sketch lists one hash twice and every record stays inside 0 < common <= u, so the stage lets it through, as it does
    # for rk_greedy_rows and rk_dbscan_rows; the collection whose records leave that range is the next test's)
    names, h, off, bits, wide, orc = collection(which)
    kmer = 24 if wide else KMER
    n = len(names)
    idx = device_index(ctx, h, off, bits, wide)
    if kernel:
        assert ctx.dist_kernel_name(idx, None, 1, metric, kmer, 0.05).startswith(kernel)
    for D, min_pts in ((0.05, 5), (0.02, 2), (0.02, 5)):   # whole clades of ten; then the clades frayed: genomes without a core record at 5
        hits = orc.hits(metric, D, kmer)
        assert len(hits) > 0
        got = ctx.mreach_rows(idx, metric, kmer, D, min_pts)
        core, edges = check(got, hits, n, min_pts, metric)
        assert got[3]["path"] == 1 and got[3]["join_attempts"] == 1
    assert any(c is None for c in core) and any(c is not None for c in core) and len(edges) > 0


def test_records_outside_the_key_are_refused(ctx, monkeypatch):
    rng = np.random.default_rng(9)
    six = np.sort(np.unique(rng.integers(0, 1 << 24, size=20))[:6])
    one = np.sort(np.concatenate([six, six[:1], six[:1]]))   # eight hashes, one of them three times
    h, off = csr([one, one])
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 1 and hits["common"][0] > hits["size0"][0] + hits["size1"][0] - hits["common"][0]   # common > u
    idx = device_index(ctx, h, off, 24)
    for leg in ("1", "0"):
        monkeypatch.setenv("RK_MREACH_DEVICE", leg)
        with pytest.raises(capi.RkError) as e:
            ctx.mreach_rows(idx, 0, KMER, 0.05, 2)
        assert e.value.code == RK_ERR_UNSUPPORTED and "common" in str(e.value)


# ---- 10. the two oracles inside the project, on the device --------------------------------------------------------------
@pytest.mark.parametrize("which,metric", [("near", 0), ("wide", 1)])
def test_min_pts_1_is_the_forest_and_the_cut_is_dbscan(ctx, which, metric):
    names, h, off, bits, wide, orc = collection(which)
    kmer = 24 if wide else KMER
    n = len(names)
    idx = device_index(ctx, h, off, bits, wide)
    core_dist, core_nb, edges, st = ctx.mreach_rows(idx, metric, kmer, 0.05, 1)
    forest, fst = ctx.forest_rows(idx, metric, kmer, 0.05)
    assert len(edges) > 0 and edges.tobytes() == forest.tobytes()   # record for record, dist and jorc bit for bit
    assert st["n_trees"] == fst["n_trees"] and not core_dist.any() and np.all(core_nb == mr.NONE) and st["max_degree"] == 0
    kinds = set()
    for min_pts in (1, 5):
        core_dist, core_nb, edges, st = ctx.mreach_rows(idx, metric, kmer, 0.05, min_pts)
        for t in (0.05, 0.03, 0.02, 0.012, 0.005):
            labels, kind, via, degree, dst = ctx.dbscan_rows(idx, metric, kmer, t, min_pts)
            want = np.where(kind == 2, labels, np.uint32(dr.NOISE))   # core labels equal, every non-core genome noise
            got = capi.mreach_cut(edges, core_dist, t)
            assert np.array_equal(got, want), (min_pts, t)
            assert np.array_equal(core_dist < t, kind == 2) and len(set(got[got != dr.NOISE].tolist())) == dst["n_clusters"]
            kinds |= set(kind.tolist())
    assert kinds == {0, 1, 2}


# ---- 11. the host leg ---------------------------------------------------------------------------------------------------
def test_host_leg_equals_the_device_path(ctx, monkeypatch):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for metric, min_pts in ((0, 5), (1, 9)):   # (at -D 0.02 the clades are frayed)
        hits = orc.hits(metric, 0.02)
        device = ctx.mreach_rows(idx, metric, KMER, 0.02, min_pts)
        check(device, hits, n, min_pts, metric)
        assert device[3]["path"] == 1 and device[3]["join_attempts"] == 1
        monkeypatch.setenv("RK_MREACH_DEVICE", "0")
        host = ctx.mreach_rows(idx, metric, KMER, 0.02, min_pts)
        monkeypatch.delenv("RK_MREACH_DEVICE")
        check(host, hits, n, min_pts, metric)
        assert host[3]["path"] == 2
        assert np.array_equal(host[0], device[0]) and np.array_equal(host[1], device[1]) and host[2].tobytes() == device[2].tobytes()
        assert all(host[3][k] == device[3][k] for k in ("n_trees", "n_core"))
        assert 0 < device[3]["n_core"] < n and device[3]["n_trees"] > 1
        rows = ctx.dist_rows(idx, None, 1, metric, KMER, 0.02)[0]   # the host rule over the join's own hit list
        again = capi.mreach_hits(rows, n, min_pts, metric)
        assert np.array_equal(again[0], device[0]) and np.array_equal(again[1], device[1]) and again[2].tobytes() == device[2].tobytes()


# ---- 12. nothing to span, and what is refused ---------------------------------------------------------------------------
def test_empty_index_single_genome_and_no_pair(ctx):
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    core_dist, core_nb, edges, st = ctx.mreach_rows(none, 0, KMER, 0.05, 3)
    assert len(core_dist) == 0 and len(edges) == 0 and st["join_attempts"] == 0 and st["path"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for min_pts, d in ((1, 0.0), (2, INF)):
        core_dist, core_nb, edges, st = ctx.mreach_rows(one, 0, KMER, 0.05, min_pts)
        assert core_dist.tolist() == [d] and core_nb.tolist() == [mr.NONE] and len(edges) == 0
        assert st["edges"] == 0 and st["n_trees"] == 1 and st["n_core"] == 2 - min_pts and st["rounds"] == 0
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 0
    idx = device_index(ctx, h, off, 24)
    check(ctx.mreach_rows(idx, 0, KMER, 0.05, 1), hits, 500, 1, 0)
    got = ctx.mreach_rows(idx, 0, KMER, 0.05, 2)
    check(got, hits, 500, 2, 0)
    assert got[3]["n_trees"] == 500 and got[3]["join_attempts"] == 1 and got[3]["rounds"] == 0


def raw_call(ctx, idx, opts, n, min_pts=3, core_dist=True, core_nb=True, edges=True, n_edges=True, stats=True):
    L = capi.lib()
    L.rk_mreach_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64), C.POINTER(capi.MreachStats)]
    bufs = [np.full(n, 77.0), np.full(n, 77, dtype=np.uint32)]
    out, count, st = C.c_void_p(), C.c_uint64(77), capi.MreachStats()
    rc = L.rk_mreach_rows(ctx._h, idx._h, C.byref(opts), min_pts, bufs[0].ctypes.data if core_dist else None, bufs[1].ctypes.data if core_nb else None,
                          C.byref(out) if edges else None, C.byref(count) if n_edges else None, C.byref(st) if stats else None)
    got = capi._take_hits(out, count) if rc == 0 else None
    return rc, bufs, got


def test_arguments_that_are_refused(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for D in (1.5, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(capi.RkError) as e:
            ctx.mreach_rows(idx, 0, KMER, D, 3)
        assert e.value.code == RK_ERR_ARG and "dense" in str(e.value)
    good = capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1)
    for opts, min_pts, text in ((capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1), 3, b"triangle"), (capi.DistOpts(1, 0, KMER, 32, 0.05, 0, 2), 3, b"row shard"),
                                (good, 0, b"min_pts")):
        rc, bufs, _ = raw_call(ctx, idx, opts, n, min_pts)
        assert rc == RK_ERR_ARG and text in capi.lib().rk_last_error(ctx._h) and all(np.all(b == 77) for b in bufs)
    with pytest.raises(capi.RkError) as e:
        ctx.mreach_rows(idx, 0, KMER, 0.05, 3, row_first=1, row_step=2, row_block=32)
    assert e.value.code == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, core_dist=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, edges=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, n_edges=False)[0] == RK_ERR_ARG
    rc, bufs, edges = raw_call(ctx, idx, good, n, core_nb=False, stats=False)   # core_nb and stats are optional
    assert rc == 0 and np.all(bufs[1] == 77)
    core, want = mr.mreach(mr.hit_tuples(orc.hits(0, 0.05)), n, 3, 0)
    assert mr.hit_tuples(edges) == want and int(np.isinf(bufs[0]).sum()) == sum(c is None for c in core)
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = orc.built
        ctx.mreach_rows(ctx.index_import(postings, counts, 24, np.diff(off)), 0, KMER, 0.05, 3)
    assert e.value.code == RK_ERR_ARG


def test_shards_of_a_sharded_build_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.mreach_rows(parts[0], 0, KMER, 0.1, 3)
    assert e.value.code == RK_ERR_ARG
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
    with pytest.raises(capi.RkError) as e:
        ctx.mreach_rows(j, 0, KMER, 0.1, 3)
    assert e.value.code == RK_ERR_ARG and "join-only" in str(e.value)
    del j, parts, sk


# ---- 13. the tool -------------------------------------------------------------------------------------------------------
def test_tool_mreach_subcommand(tmp_path):
    names, h, off, bits, wide, orc = collection("near")
    assert bits == 24 and len(set(names)) == len(names)
    synth.write_sketch_file(str(tmp_path / "near.sketch"), 10, 6, 4, names, h, off)   # 4 * (10 - 4) = 24 bits, k = 20
    n = len(names)
    for metric, min_pts, t in ((0, 5, 0.012), (1, 9, 0.02)):
        hits = orc.hits(metric, 0.02)
        tuples = mr.hit_tuples(hits)
        at = {x[:2]: i for i, x in enumerate(tuples)}
        core, edges = mr.mreach(tuples, n, min_pts, metric)
        assert any(c is None for c in core) and len(edges) > 100
        core_dist = [INF if c is None else float(hits["dist"][at[c[0][:2]]]) for c in core]
        recs = hits[[at[e[:2]] for e in edges]]
        mw = [max(float(r["dist"]), core_dist[r["row"]], core_dist[r["col"]]) for r in recs]
        below = hits[hits["dist"] < t]
        labels, kind, _, _ = dr.dbscan(dr.hit_tuples(below), n, min_pts, metric)
        labels = [l if k == dr.KIND_CORE else mr.NOISE for l, k in zip(labels, kind)]
        assert len(set(labels)) > 3 and mr.NOISE in labels
        out, cf, lf = (tmp_path / (name % metric) for name in ("m%d.txt", "core%d.txt", "labels%d.txt"))
        p = subprocess.run([TOOL, "mreach", "-i", "near.sketch", "-D", "0.02", "-M", str(metric), "-m", str(min_pts), "-o", out.name, "--core", cf.name,
                            "--cut", repr(t), "--labels", lf.name], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert out.read_text() == mr.render_edges(names, recs, mw), (metric, min_pts)
        assert cf.read_text() == mr.render_core(names, core_dist, [mr.NONE if c is None else c[1] for c in core])
        assert lf.read_text() == mr.render_labels(names, labels)
    p = subprocess.run([TOOL, "mreach", "-i", "near.sketch", "-D", "0.05", "-m", "5", "-o", "two.txt", "--gpus", "2"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"mreach runs on one GPU" in p.stderr and not (tmp_path / "two.txt").exists()
    for extra, text in (([], b"minPts must be >= 1"), (["-m", "0"], b"minPts must be >= 1"), (["-m", "3", "--cut", "0.01"], b"go together"),
                        (["-m", "3", "--cut", "0.06", "--labels", "l.txt"], b"--cut must lie")):
        p = subprocess.run([TOOL, "mreach", "-i", "near.sketch", "-D", "0.05", "-o", "none.txt"] + extra, cwd=tmp_path, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode != 0 and text in p.stderr and not (tmp_path / "none.txt").exists()
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"mreach -i" in p.stderr and b" dbscan mreach " in p.stderr
