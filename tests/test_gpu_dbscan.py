"""rk_dbscan_rows: the density-based clusters of the self join against tests/_dbscan_ref.py (exact rational ratios, adjacency sets, a
breadth-first search) over the ORACLE's hit list, set up from tests/_selfjoin_cases.py (its Oracle, device_index and collections, built
once per session): labels, kinds, via and degrees, exactly.  Every case says from the call's stats that it reached the edge it is
about."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import _dbscan_ref as dr
from _selfjoin_cases import (KMER, TOOL, Oracle, both_overflows_collection, both_overflows_thresholds, collection, csr, device_index,
                             identical, permuted)
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
RK_ERR_ARG = -1
NOISE, BORDER, CORE = dr.KIND_NOISE, dr.KIND_BORDER, dr.KIND_CORE


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def check(got, hits, n, min_pts, metric):
    """(labels, kind, via, degree, stats) of one call against the reference over the oracle's hit list `hits`; returns the reference's
    (labels, kind, via, degree)"""
    want = dr.dbscan(dr.hit_tuples(hits), n, min_pts, metric)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint8 and got[2].dtype == np.uint32 and got[3].dtype == np.uint32
    for mine, ref, what in zip(got, want, ("labels", "kind", "via", "degree")):
        assert np.array_equal(mine, np.array(ref, dtype=mine.dtype)), what
    st = got[4]
    assert (st["n_core"], st["n_border"], st["n_noise"]) == tuple(want[1].count(k) for k in (CORE, BORDER, NOISE))
    assert st["n_clusters"] == len({l for l, k in zip(want[0], want[1]) if k == CORE})
    assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
    assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(hits)   # the device consumed exactly the oracle's pairs
    return want


# ---- 1. the comparator: every pair at distance 0 ------------------------------------------------------------------------
def test_identical_sketches_are_all_core_or_all_noise(ctx):
    h, off = csr(permuted(identical(300, 2), 12))
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 300 * 299 // 2 and np.all(hits["dist"] == 0.0)
    idx = device_index(ctx, h, off, 24)
    got = ctx.dbscan_rows(idx, 0, KMER, 0.05, 300)   # deg + 1 == min_pts: core at equality
    check(got, hits, 300, 300, 0)
    assert not got[0].any() and np.all(got[1] == CORE) and np.all(got[3] == 299) and got[4]["n_clusters"] == 1 and got[4]["n_core"] == 300
    got = ctx.dbscan_rows(idx, 0, KMER, 0.05, 301)
    check(got, hits, 300, 301, 0)
    assert np.all(got[0] == dr.NOISE) and np.all(got[2] == dr.NOISE) and not got[1].any() and got[4]["n_clusters"] == 0 and got[4]["n_noise"] == 300


# ---- 2. chaining: the case the feature exists for -----------------------------------------------------------------------
def chain_parts(seed, equal):
    """([A, B, x], the rest): two groups of g = 3 identical sketches A and B that share nothing, their satellites (five per group, each
    with the part of its group's sketch that x does not touch: adjacent to the group and to each other, never to x), and x, which holds
    hashes of both groups' sketches.  The rest: the other two copies of A and of B, then the satellites.
    equal: |A| = 35, |B| = 55, |x| = 45 with 20 of A and 25 of B -- jaccard 20/60 = 25/75, d = 0.0347 both; satellites at 15/40 and 30/65.
    else : 100 hashes each, x with 40 of A (40/160, d = 0.0458) and 30 of B (30/170, d = 0.0602); satellites at 60/140.
    deg(x) = 6, deg(a copy) = 2 + 1 + 5 = 8, deg(a satellite) = 3 + 4 = 7: at min_pts 8 everything but x is core."""
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


def test_a_genome_between_two_groups_does_not_chain_them(ctx):
    first, rest = chain_parts(7, equal=False)
    order = np.random.default_rng(8).permutation(3 + len(rest))
    parts = first + rest
    h, off = csr([parts[i] for i in order])
    n = len(parts)
    where = {int(src): at for at, src in enumerate(order)}
    x, a_copies, b_copies = where[2], sorted(where[i] for i in (0, 3, 4)), sorted(where[i] for i in (1, 5, 6))
    hits = Oracle(h, off, 24).hits(0, 0.07)
    idx = device_index(ctx, h, off, 24)
    got = ctx.dbscan_rows(idx, 0, KMER, 0.07, 8)
    check(got, hits, n, 8, 0)
    labels, kind, via, degree, st = got
    assert degree[x] == 6 and kind[x] == BORDER and st["n_core"] == n - 1 and st["n_border"] == 1 and st["n_clusters"] == 2
    assert via[x] == a_copies[0] and labels[x] == labels[a_copies[0]] != labels[b_copies[0]]   # the nearer group, its smallest copy
    single, cst = ctx.cluster_rows(idx, 0, KMER, 0.07)
    assert cst["n_clusters"] == 1 and not single.any()   # single linkage chains the two groups through x


@pytest.mark.parametrize("roles", list(itertools.permutations(range(3))))
def test_equal_ratio_from_different_counts_goes_to_the_smaller_core_index(ctx, roles):
    first, rest = chain_parts(9, equal=True)
    h, off = csr([first[r] for r in roles] + rest)   # the first copy of A, the first of B and x at the caller indices 0, 1, 2 in every order
    n = 3 + len(rest)
    a, b, x = roles.index(0), roles.index(1), roles.index(2)
    hits = Oracle(h, off, 24).hits(0, 0.07)
    tuples = {t[:2]: t for t in dr.hit_tuples(hits)}
    ta, tb = tuples[(min(a, x), max(a, x))], tuples[(min(b, x), max(b, x))]
    assert (ta[2], tb[2]) == (20, 25) and ta[2] * (tb[3] + tb[4] - tb[2]) == tb[2] * (ta[3] + ta[4] - ta[2])   # 20/60 == 25/75
    idx = device_index(ctx, h, off, 24)
    got = ctx.dbscan_rows(idx, 0, KMER, 0.07, 8)
    check(got, hits, n, 8, 0)
    labels, kind, via, degree, st = got
    assert kind[x] == BORDER and degree[x] == 6 and via[x] == min(a, b) and labels[x] == labels[min(a, b)] and st["n_clusters"] == 2
    assert ctx.cluster_rows(idx, 0, KMER, 0.07)[1]["n_clusters"] == 1


# ---- 3. union-find depth: a path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["identity", "permuted"])
def test_path_of_2000_genomes(ctx, order):
    # the path of the cluster suite (neighbours share 95 of 100: d = 0.00256, next but one 0.00527) over 24-bit hashes: the oracle's
    # index of 2^28 counters alone takes seconds
    n, m, step = 2000, 100, 5
    rng = np.random.default_rng(1)
    pool = np.unique(rng.integers(0, 1 << 24, size=step * n + m + 4000))[: step * (n - 1) + m]
    assert len(pool) == step * (n - 1) + m
    parts = [pool[step * i: step * i + m] for i in range(n)]
    ends = [0, n - 1]
    if order == "permuted":
        perm = np.random.default_rng(11).permutation(n)
        parts = [parts[i] for i in perm]
        ends = [int(np.flatnonzero(perm == e)[0]) for e in ends]
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.004)
    assert len(hits) == n - 1
    idx = device_index(ctx, h, off, 24)
    got = ctx.dbscan_rows(idx, 0, KMER, 0.004, 3)
    check(got, hits, n, 3, 0)
    labels, kind, via, degree, st = got
    assert st["n_clusters"] == 1 and st["n_core"] == n - 2 and st["n_border"] == 2 and st["join_attempts"] == 1 and st["border_attempts"] == 1
    assert sorted(np.flatnonzero(kind == BORDER).tolist()) == sorted(ends) and len(set(labels.tolist())) == 1
    assert int(labels[0]) == min(i for i in range(n) if i not in ends)   # the smallest CORE index
    got = ctx.dbscan_rows(idx, 0, KMER, 0.004, 4)
    check(got, hits, n, 4, 0)
    assert got[4]["n_noise"] == n and got[4]["n_clusters"] == 0 and np.all(got[0] == dr.NOISE)


# ---- 4. contention: a star ----------------------------------------------------------------------------------------------
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
    got = ctx.dbscan_rows(idx, 0, KMER, 0.03, 3)
    check(got, hits, 3001, 3, 0)
    labels, kind, via, degree, st = got
    leaves = np.arange(3001) != centre
    assert kind[centre] == CORE and degree[centre] == 3000 and np.all(kind[leaves] == BORDER) and np.all(via[leaves] == centre)
    assert np.all(labels == centre) and (st["n_clusters"], st["n_core"], st["n_border"]) == (1, 1, 3000)
    got = ctx.dbscan_rows(idx, 0, KMER, 0.03, 2)
    check(got, hits, 3001, 2, 0)
    assert np.all(got[1] == CORE) and np.all(got[0] == 0) and got[4]["n_clusters"] == 1


# ---- 5. the borderline edge that decides a core, and both overflows -----------------------------------------------------
def test_borderline_records_decide_cores_behind_both_overflows(ctx, monkeypatch):
    h, off = both_overflows_collection()
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    for D, n_hits, kept in both_overflows_thresholds():
        hits = orc.hits(0, D)
        assert len(hits) == n_hits > 65536
        got = ctx.dbscan_rows(idx, 0, KMER, D, 2)
        check(got, hits, 420, 2, 0)
        st = got[4]
        assert st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        # one ulp above: ten clusters of two beside the clique; on the distance itself: twenty noise genomes
        assert (st["n_clusters"], st["n_core"], st["n_border"], st["n_noise"]) == ((11, 420, 0, 0) if kept else (1, 400, 0, 20))
        sizes = sorted(np.bincount(got[0][got[1] == CORE]).tolist())
        assert [s for s in sizes if s] == ([2] * 10 + [400] if kept else [400])


# ---- 6. a borderline cascade --------------------------------------------------------------------------------------------
def cascade_collection():
    """Two clusters P and Q, each a sketch P0 / Q0 of 100 hashes and three copies of a sketch that holds 65 of its hashes; g holds the
    other 35 of P0, the other 35 of Q0 and 30 of its own (g - P0 and g - Q0 at 35/165, d = 0.0525), z those 30 and 70 of its own (z - g
    at 30/170: the distance of both_overflows' kind, -ln(0.3) / 20 = 0.0602).  deg(g) = 2 without z: at min_pts 4 the edge z - g makes g
    core, and a core g joins P and Q.  Returns (h, off, g, z, p0, q0) in a fixed random caller order."""
    rng = np.random.default_rng(23)
    pool = np.unique(rng.integers(0, 1 << 24, size=1000))
    rng.shuffle(pool)
    P0, Q0, own, zown, pown, qown = pool[:100], pool[100:200], pool[200:230], pool[230:300], pool[300:335], pool[335:370]
    g = np.concatenate([P0[:35], Q0[:35], own])
    z = np.concatenate([own, zown])
    P1, Q1 = np.concatenate([P0[35:], pown]), np.concatenate([Q0[35:], qown])
    parts = [np.sort(p) for p in (g, z, P0, Q0, P1, P1, P1, Q1, Q1, Q1)]
    order = np.random.default_rng(24).permutation(len(parts))
    h, off = csr([parts[i] for i in order])
    where = [int(np.flatnonzero(order == i)[0]) for i in range(4)]
    return (h, off) + tuple(where)


@pytest.mark.parametrize("metric", [0, 1])
def test_borderline_edge_makes_a_core_that_joins_two_clusters(ctx, metric):
    h, off, g, z, p0, q0 = cascade_collection()
    n = len(off) - 1
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    for D, joined in ((float(np.nextafter(d0, 0.0)), False), (d0, False), (float(np.nextafter(d0, 1.0)), True)):   # strict <
        hits = orc.hits(metric, D)
        assert ((min(g, z), max(g, z)) in {t[:2] for t in dr.hit_tuples(hits)}) == joined   # where the oracle's hit list flips
        got = ctx.dbscan_rows(idx, metric, KMER, D, 4)
        check(got, hits, n, 4, metric)
        labels, kind, via, degree, st = got
        assert st["borderline"] >= 1 and st["borderline_kept"] == int(joined) and st["n_clusters"] == (1 if joined else 2)
        assert degree[g] == 2 + int(joined) and kind[g] == (CORE if joined else BORDER) and kind[z] == (BORDER if joined else NOISE)
        if joined:
            assert via[z] == g and len(set(labels.tolist())) == 1
        else:
            assert via[g] == min(p0, q0) and labels[p0] != labels[q0] and labels[z] == dr.NOISE   # g - P0 ties g - Q0: the smaller index


# ---- 7. every kernel of the join, both metrics, 36-bit hashes -----------------------------------------------------------
@pytest.mark.parametrize("which,kernel,metric", [
    ("tiles", "rk_tile_kernel", 0), ("tiles", "rk_tile_kernel", 1), ("near", "rk_near_kernel", 0), ("near", "rk_near_kernel", 1),
    ("repeat", "rk_dist_kernel", 0), ("repeat", "rk_dist_kernel", 1), ("wide", None, 0), ("wide", None, 1)])
def test_every_join_kernel_both_metrics_and_wide_hashes(ctx, which, kernel, metric):
    names, h, off, bits, wide, orc = collection(which)
    kmer = 24 if wide else KMER
    n = len(names)
    idx = device_index(ctx, h, off, bits, wide)
    if kernel:
        assert ctx.dist_kernel_name(idx, None, 1, metric, kmer, 0.05).startswith(kernel)
    for D in (0.05, 0.02):   # whole clades of ten, every genome core up to min_pts 10; then the clades frayed: all three kinds at 5
        hits = orc.hits(metric, D, kmer)
        assert len(hits) > 0
        for min_pts in (1, 2, 5):
            got = ctx.dbscan_rows(idx, metric, kmer, D, min_pts)
            want = check(got, hits, n, min_pts, metric)
            if min_pts == 1:
                single, cst = ctx.cluster_rows(idx, metric, kmer, D)
                assert np.array_equal(got[0], single) and got[4]["n_clusters"] == cst["n_clusters"] and got[4]["n_core"] == n
        assert set(want[1]) == ({NOISE, BORDER, CORE} if D == 0.02 else {CORE} if which != "repeat" else {NOISE, CORE})


# ---- 8. the fallback ----------------------------------------------------------------------------------------------------
def test_host_fallback_equals_the_device_path(ctx, monkeypatch):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for metric, min_pts in ((0, 5), (1, 9)):   # (at -D 0.02 the clades are frayed: all three kinds)
        hits = orc.hits(metric, 0.02)
        device = ctx.dbscan_rows(idx, metric, KMER, 0.02, min_pts)
        check(device, hits, n, min_pts, metric)
        assert device[4]["join_attempts"] == 1
        monkeypatch.setenv("RK_DBSCAN_DEVICE", "0")
        host = ctx.dbscan_rows(idx, metric, KMER, 0.02, min_pts)
        monkeypatch.delenv("RK_DBSCAN_DEVICE")
        check(host, hits, n, min_pts, metric)
        assert host[4]["join_attempts"] == 0 and host[4]["edges"] == len(hits)
        assert all(np.array_equal(a, b) for a, b in zip(host[:4], device[:4]))
        assert all(host[4][k] == device[4][k] for k in ("n_clusters", "n_core", "n_border", "n_noise"))
        assert device[4]["n_noise"] and device[4]["n_border"] and device[4]["n_clusters"] > 1
        rows = ctx.dist_rows(idx, None, 1, metric, KMER, 0.02)[0]   # the host rule over the join's own hit list
        assert all(np.array_equal(a, b) for a, b in zip(capi.dbscan_hits(rows, n, min_pts, metric), device[:4]))


# ---- 9. nothing to cluster, and what is refused -------------------------------------------------------------------------
def test_empty_index_single_genome_and_no_pair(ctx):
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    labels, kind, via, degree, st = ctx.dbscan_rows(none, 0, KMER, 0.05, 3)
    assert len(labels) == 0 and st["join_attempts"] == 0 and st["n_clusters"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for min_pts, core in ((1, True), (2, False)):
        labels, kind, via, degree, st = ctx.dbscan_rows(one, 0, KMER, 0.05, min_pts)
        assert labels.tolist() == [0 if core else dr.NOISE] and kind.tolist() == [CORE if core else NOISE] and via.tolist() == [dr.NOISE]
        assert degree.tolist() == [0] and st["edges"] == 0 and st["n_clusters"] == int(core)
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 0
    idx = device_index(ctx, h, off, 24)
    check(ctx.dbscan_rows(idx, 0, KMER, 0.05, 1), hits, 500, 1, 0)
    got = ctx.dbscan_rows(idx, 0, KMER, 0.05, 2)
    check(got, hits, 500, 2, 0)
    assert got[4]["n_noise"] == 500 and got[4]["join_attempts"] == 1


def raw_call(ctx, idx, opts, n, min_pts=3, labels=True, kind=True, via=True, degree=True, stats=True):
    L = capi.lib()
    L.rk_dbscan_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(capi.DbscanStats)]
    bufs = [np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint8), np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint32)]
    st = capi.DbscanStats()
    rc = L.rk_dbscan_rows(ctx._h, idx._h, C.byref(opts), min_pts, *[b.ctypes.data if on else None for b, on in zip(bufs, (labels, kind, via, degree))],
                          C.byref(st) if stats else None)
    return rc, bufs


def test_arguments_that_are_refused(ctx):
    names, h, off, bits, wide, orc = collection("repeat")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for D in (1.5, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(capi.RkError) as e:
            ctx.dbscan_rows(idx, 0, KMER, D, 3)
        assert e.value.code == RK_ERR_ARG and "dense" in str(e.value)
    check(ctx.dbscan_rows(idx, 0, KMER, 1.0, 3), orc.hits(0, 1.0), n, 3, 0)   # the default -D 1.0 of alldist stays sparse
    good = capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1)
    for opts, min_pts, text in ((capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1), 3, b"triangle"), (capi.DistOpts(1, 0, KMER, 32, 0.05, 0, 2), 3, b"row shard"),
                                (good, 0, b"min_pts")):
        rc, bufs = raw_call(ctx, idx, opts, n, min_pts)
        assert rc == RK_ERR_ARG and text in capi.lib().rk_last_error(ctx._h) and all(np.all(b == 77) for b in bufs)
    with pytest.raises(capi.RkError) as e:
        ctx.dbscan_rows(idx, 0, KMER, 0.05, 3, row_first=1, row_step=2, row_block=32)
    assert e.value.code == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, labels=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, kind=False)[0] == RK_ERR_ARG
    rc, bufs = raw_call(ctx, idx, good, n, via=False, degree=False, stats=False)   # via, degree and stats are optional
    assert rc == 0 and np.all(bufs[2] == 77) and np.all(bufs[3] == 77)
    assert bufs[0].tolist() == dr.dbscan(dr.hit_tuples(orc.hits(0, 0.05)), n, 3, 0)[0]
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = orc.built
        ctx.dbscan_rows(ctx.index_import(postings, counts, 24, np.diff(off)), 0, KMER, 0.05, 3)
    assert e.value.code == RK_ERR_ARG


def test_shards_of_a_sharded_build_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.dbscan_rows(parts[0], 0, KMER, 0.1, 3)
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
    _, st = ctx.cluster_rows(j, 0, KMER, 0.1)   # single linkage accepts the join-only index: it holds the rows of shard 0
    assert st["edges"] > 0
    with pytest.raises(capi.RkError) as e:
        ctx.dbscan_rows(j, 0, KMER, 0.1, 3)
    assert e.value.code == RK_ERR_ARG and "join-only" in str(e.value)
    del j, parts, sk


# ---- 10. the tool -------------------------------------------------------------------------------------------------------
def test_tool_dbscan_subcommand(tmp_path):
    names, h, off, bits, wide, orc = collection("near")
    assert bits == 24 and len(set(names)) == len(names)
    synth.write_sketch_file(str(tmp_path / "near.sketch"), 10, 6, 4, names, h, off)   # 4 * (10 - 4) = 24 bits, k = 20
    n = len(names)
    for metric, min_pts in ((0, 5), (1, 9)):
        want = dr.dbscan(dr.hit_tuples(orc.hits(metric, 0.02)), n, min_pts, metric)
        assert {NOISE, BORDER, CORE} == set(want[1])
        text = dr.render(names, *want)
        out = tmp_path / ("d%d.txt" % metric)
        p = subprocess.run([TOOL, "dbscan", "-i", "near.sketch", "-D", "0.02", "-M", str(metric), "-m", str(min_pts), "-o", out.name], cwd=tmp_path,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert out.read_text() == text, (metric, min_pts)
    p = subprocess.run([TOOL, "dbscan", "-i", "near.sketch", "-D", "0.05", "-m", "5", "-o", "two.txt", "--gpus", "2"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"dbscan runs on one GPU" in p.stderr and not (tmp_path / "two.txt").exists()
    for extra in ([], ["-m", "0"]):
        p = subprocess.run([TOOL, "dbscan", "-i", "near.sketch", "-D", "0.05", "-o", "none.txt"] + extra, cwd=tmp_path, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode != 0 and b"minPts must be >= 1" in p.stderr and not (tmp_path / "none.txt").exists()
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"dbscan -i" in p.stderr and b" knn dbscan " in p.stderr
