"""rk_knn_rows: the k nearest neighbours of every genome against tests/_knn_ref.py (exact rational ratios) over the ORACLE's hit list,
set up from tests/_selfjoin_cases.py (its Oracle, device_index and collections, built once per session): the
offsets, the exact record tuples, and jorc / dist bit for bit.  Every case says from the call's stats that it reached the edge it is
about."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _knn_ref as kr
from _selfjoin_cases import (KMER, TOOL, Oracle, borderline_overflow_collection, both_overflows_collection, both_overflows_thresholds,
                             bridge_collection, collection, csr, device_index, hit_overflow_collection, identical, permuted,
                             tie_collection, trio)
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
RK_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def check_lists(off, nbrs, hits, n, k, metric):
    """offsets and records (of a call or of a fold) against the reference over the oracle's hit list `hits`; returns its lists"""
    want = kr.knn(kr.hit_tuples(hits), n, k, metric)
    assert off.dtype == np.uint64 and off.tolist() == kr.offsets(want)
    flat = kr.flat(want)
    assert kr.hit_tuples(nbrs) == flat
    value = {(int(r), int(c)): (float(j), float(d)) for r, c, j, d in zip(hits["row"], hits["col"], hits["jorc"], hits["dist"])}
    assert np.array_equal(nbrs["jorc"], np.array([value[h[:2]][0] for h in flat], dtype=np.float64))
    assert np.array_equal(nbrs["dist"], np.array([value[h[:2]][1] for h in flat], dtype=np.float64))
    assert np.all(nbrs["row"] < nbrs["col"])
    return want


def check(got, hits, n, k, metric, shard_hits=None):
    """(off, nbrs, stats) of one call against the oracle's hit list (shard_hits: the records this call's row shard owns)"""
    off, nbrs, st = got
    mine = hits if shard_hits is None else shard_hits
    want = check_lists(off, nbrs, mine, n, k, metric)
    assert st["neighbours"] == len(nbrs) == sum(len(one) for one in want)
    assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
    assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(mine)   # the device consumed exactly the oracle's pairs
    return want


def degrees(hits, n):
    return np.bincount(np.concatenate([hits["row"], hits["col"]]).astype(np.int64), minlength=n)


# ---- 1. every pair at distance 0 ----------------------------------------------------------------------------------------
def test_all_ties_give_the_smallest_indices(ctx):
    h, off = csr(permuted(identical(300, 2), 12))
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 300 * 299 // 2 and np.all(hits["dist"] == 0.0)
    got = ctx.knn_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, 5)
    want = check(got, hits, 300, 5, 0)
    st = got[2]
    assert st["path"] == 1 and st["max_degree"] == 299 and st["edges"] == 44850 and st["neighbours"] == 1500   # five chunks of equal keys per genome
    for v in range(300):
        assert [kr.other(r, v) for r in want[v]] == [i for i in range(6) if i != v][:5]


# ---- 2. degrees at the seam between two chunks --------------------------------------------------------------------------
_cliques = {}


def cliques():
    """cliques of 64, 65, 66 and 129 sketches: 100 hashes each, 80 .. 95 of them from the clique's 100 (any two share 60 or more:
    d <= -ln(2 * 60/140 / (1 + 60/140)) / 20 = 0.026), in a fixed random caller order"""
    if not _cliques:
        rng = np.random.default_rng(41)
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
        h, off = csr(permuted(parts, 42))
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
    got = ctx.knn_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, k)
    want = check(got, hits, n, k, 0)
    assert got[2]["path"] == 1 and got[2]["max_degree"] == 128 and got[2]["join_attempts"] == 1
    assert {len(one) for one in want} == ({k} if k < 64 else {63, 64})


# ---- 3. a path: lists shorter than k, empty lists ---------------------------------------------------------------------
_path = {}


def path():
    """the path of test_path_of_2048_genomes (genome i + 1 keeps 50 .. 95 of genome i's 100 hashes) and five unrelated sketches,
    in a fixed random caller order; at -D 0.02 (67 shared hashes or more) the path falls into pieces"""
    if not _path:
        n, m = 2048, 100
        rng = np.random.default_rng(1)
        share = rng.integers(50, 96, size=n - 1)
        pool = np.unique(rng.integers(0, 1 << 24, size=130000))
        rng.shuffle(pool)
        parts, used = [pool[:m]], m
        for i in range(n - 1):
            fresh = m - int(share[i])
            parts.append(np.concatenate([rng.choice(parts[-1], size=int(share[i]), replace=False), pool[used: used + fresh]]))
            used += fresh
        parts += [pool[used + m * j: used + m * j + m] for j in range(5)]
        h, off = csr(permuted([np.sort(p) for p in parts], 11))
        _path["it"] = (h, off, Oracle(h, off, 24))
    return _path["it"]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_path_with_short_and_empty_lists(ctx, k):
    h, off, orc = path()
    n = len(off) - 1
    hits = orc.hits(0, 0.02)
    deg = degrees(hits, n)
    assert n == 2053 and int((deg == 0).sum()) >= 5 and int((deg == 1).sum()) > 100 and int((deg == 2).sum()) > 100 and len(hits) > 1000
    got = ctx.knn_rows(device_index(ctx, h, off, 24), 0, KMER, 0.02, k)
    want = check(got, hits, n, k, 0)
    assert got[2]["path"] == 1 and got[2]["max_degree"] == int(deg.max())
    lengths = [len(one) for one in want]
    assert 0 in lengths and (k == 1 or any(0 < x < k for x in lengths))
    assert int((np.diff(got[0]) == 0).sum()) == int((deg == 0).sum())   # offsets that repeat


# ---- 4. a star: one heavy genome ----------------------------------------------------------------------------------------
def test_star_of_3000_leaves(ctx):
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=140000))
    rng.shuffle(pool)
    hub, spare = pool[:100], pool[100:]
    parts = [np.sort(hub)]
    for j in range(3000):   # a leaf: 60 of the hub's hashes and 40 of its own -- hub-leaf d = 0.0255, leaf-leaf ~0.05
        parts.append(np.sort(np.concatenate([rng.choice(hub, size=60, replace=False), spare[40 * j: 40 * j + 40]])))
    order = np.random.default_rng(12).permutation(3001)
    h, off = csr([parts[i] for i in order])
    centre = int(np.flatnonzero(order == 0)[0])
    hits = Oracle(h, off, 24).hits(0, 0.03)
    deg = degrees(hits, 3001)
    assert deg[centre] == 3000 == deg.max() and int((deg == 1).sum()) > 2000
    got = ctx.knn_rows(device_index(ctx, h, off, 24), 0, KMER, 0.03, 10)
    want = check(got, hits, 3001, 10, 0)
    assert got[2]["path"] == 1 and got[2]["max_degree"] == 3000   # the hub's segment: 47 chunks
    assert len(want[centre]) == 10 and [kr.other(r, centre) for r in want[centre]] == sorted(kr.other(r, centre) for r in want[centre])   # (all at 60/140)


# ---- 5. one ratio from different counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_equal_ratio_from_different_counts(ctx, metric):
    # the member's 30 hashes; metric 0: 20 of them in a sketch of 50 (20/60) and 25 in one of 70 (25/75); metric 1: 16 in a sketch of
    # 24 (16/24) and 20 in one of 70 (20/30).  The member's nearest neighbour is the smaller index, whichever count that is
    sizes, shares = ((50, 70, 30), (20, 25)) if metric == 0 else ((24, 70, 30), (16, 20))
    for roles in ((0, 1, 2), (1, 0, 2)):
        h, off = trio(3, sizes, shares, roles)
        hits = Oracle(h, off, 24).hits(metric, 0.05)
        tuples = kr.hit_tuples(hits)
        assert [t[:2] for t in tuples] == [(0, 2), (1, 2)] and tuples[0][2] != tuples[1][2]
        assert kr.place(tuples[0], 2, metric)[1] == kr.place(tuples[1], 2, metric)[1]
        got = ctx.knn_rows(device_index(ctx, h, off, 24), metric, KMER, 0.05, 1)
        want = check(got, hits, 3, 1, metric)
        assert want == [[tuples[0]], [tuples[1]], [tuples[0]]] and got[2]["path"] == 1
    h, off = tie_collection(3)   # six triangles, one per assignment of the roles to ascending indices, and six plain pairs
    n = len(off) - 1
    hits = Oracle(h, off, 24).hits(metric, 0.06)
    two = kr.knn(kr.hit_tuples(hits), n, 2, metric)
    tied = [v for v in range(n) if len(two[v]) == 2 and kr.place(two[v][0], v, metric)[1] == kr.place(two[v][1], v, metric)[1]]
    if metric == 0:
        assert len(tied) == 18 and any(two[v][0][2] != two[v][1][2] for v in tied)
    got = ctx.knn_rows(device_index(ctx, h, off, 24), metric, KMER, 0.06, 1)
    want = check(got, hits, n, 1, metric)
    for v in tied:
        assert kr.other(want[v][0], v) < kr.other(two[v][1], v)


# ---- 6. a pair exactly on the threshold, and one ulp either side --------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_bridge_on_the_threshold_and_one_ulp_either_side(ctx, metric):
    h, off = bridge_collection(2, 5)   # A, B, then a (70 of A's hashes) and b (70 of B's), who share 30 others: the bridge
    n = len(off) - 1
    a, b = n - 2, n - 1
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    for D, bridged in ((float(np.nextafter(d0, 0.0)), False), (d0, False), (float(np.nextafter(d0, 1.0)), True)):   # strict <
        hits = orc.hits(metric, D)
        assert len(hits) == 2 + int(bridged)
        for k in (1, 2):
            got = ctx.knn_rows(idx, metric, KMER, D, k)
            want = check(got, hits, n, k, metric)
            st = got[2]
            assert st["borderline"] >= 1 and st["borderline_kept"] == int(bridged) and st["path"] == 1
            in_a, in_b = [(a, b) in [r[:2] for r in want[v]] for v in (a, b)]
            assert in_a == in_b == (bridged and k == 2)   # kept, it enters a list that has room and never displaces the nearer neighbour
            assert [kr.other(r, a) for r in want[a]][0] < a and [kr.other(r, b) for r in want[b]][0] < a
            assert st["neighbours"] == (4 if k == 1 else 4 + 2 * int(bridged))


# ---- 7. overflows -------------------------------------------------------------------------------------------------------
def test_hit_buffer_overflow_runs_the_join_again(ctx):
    h, off = hit_overflow_collection()
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 400 * 399 // 2 > max(65536, 403 * 64)
    got = ctx.knn_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, 3)
    check(got, hits, 403, 3, 0)
    st = got[2]
    assert st["join_attempts"] == 2 and st["edges"] == len(hits) and st["max_degree"] == 399 and st["neighbours"] == 1200 and st["path"] == 1


def test_borderline_overflow_runs_the_key_pass_again(ctx, monkeypatch):
    h, off = borderline_overflow_collection()
    _, d0 = ok.distance(80, 100, 100, 0, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "1")
    up = float(np.nextafter(d0, 1.0))
    got = ctx.knn_rows(idx, 0, KMER, up, 2)
    check(got, orc.hits(0, up), 600, 2, 0)
    st = got[2]
    assert st["border_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 300 and st["neighbours"] == 600 and st["max_degree"] == 0
    got = ctx.knn_rows(idx, 0, KMER, d0, 2)
    check(got, orc.hits(0, d0), 600, 2, 0)
    st = got[2]
    assert st["border_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 0 and st["neighbours"] == 0 and len(got[1]) == 0


def test_hit_and_borderline_overflow_in_one_call(ctx, monkeypatch):
    h, off = both_overflows_collection()
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    for D, n_hits, kept in both_overflows_thresholds():
        hits = orc.hits(0, D)
        assert len(hits) == n_hits
        got = ctx.knn_rows(idx, 0, KMER, D, 2)
        check(got, hits, 420, 2, 0)
        st = got[2]
        assert st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        assert st["neighbours"] == 800 + 2 * kept and st["max_degree"] == 399


# ---- 8. every kernel of the join, both metrics, 36-bit hashes -----------------------------------------------------------
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
    hits = orc.hits(metric, 0.05, kmer)
    got = ctx.knn_rows(idx, metric, kmer, 0.05, 3)
    want = check(got, hits, n, 3, metric)
    st = got[2]
    assert st["path"] == 1 and st["edges"] >= len(hits) > 0 and st["max_degree"] == int(degrees(hits, n).max()) > 3
    assert 0 < st["neighbours"] < 2 * len(hits) and max(len(one) for one in want) == 3


# ---- 9. shards ----------------------------------------------------------------------------------------------------------
def test_three_row_shards_fold_to_the_whole(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    hits = orc.hits(0, 0.05)
    for k in (1, 4):
        whole = ctx.knn_rows(idx, 0, KMER, 0.05, k)
        check(whole, hits, n, k, 0)
        owner = idx.shard_of(hits, 3, 32)
        folded = (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=capi.HIT_DTYPE))
        for first in range(3):
            part = ctx.knn_rows(idx, 0, KMER, 0.05, k, row_first=first, row_step=3, row_block=32)
            assert 0 < len(part[1]) < len(whole[1]) and part[2]["path"] == 1
            check(part, hits, n, k, 0, shard_hits=hits[owner == first])   # one shard alone: the first k of the records it owns
            folded = capi.knn_merge(folded[0], folded[1], part[0], part[1], n, k, 0)
        check_lists(folded[0], folded[1], hits, n, k, 0)
        assert np.array_equal(folded[0], whole[0])
        for f in capi.HIT_DTYPE.names:
            assert np.array_equal(folded[1][f], whole[1][f]), f


def test_join_only_indexes_of_a_two_shard_build_fold_to_the_whole(ctx):
    import torch
    S, k = 2, 4
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=S))
    n = len(names)
    hits = Oracle(h, off, 20).hits(0, 0.1)
    assert len(hits) > 1000
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.knn_rows(parts[0], 0, KMER, 0.1, k)
    assert e.value.code == RK_ERR_ARG
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    folded = (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=capi.HIT_DTYPE))
    consumed = 0
    for d in range(S):   # the shards played in turn
        recv = torch.cat([bufs[r][12 * sum(sent[r][:d]): 12 * sum(sent[r][:d + 1])] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        j = ctx.index_join_shard(parts[d], recv.data_ptr(), sum(sent[r][d] for r in range(S)))
        part = ctx.knn_rows(j, 0, KMER, 0.1, k)
        assert part[2]["path"] == 1
        consumed += part[2]["edges"] - part[2]["borderline"] + part[2]["borderline_kept"]
        folded = capi.knn_merge(folded[0], folded[1], part[0], part[1], n, k, 0)
        del j
    assert consumed == len(hits)
    check_lists(folded[0], folded[1], hits, n, k, 0)
    del parts, sk


# ---- 10. the paths around the device selection --------------------------------------------------------------------------
def test_fallback_paths(ctx, monkeypatch):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    hits = orc.hits(0, 0.05)
    off0, nbrs0, st = ctx.knn_rows(idx, 0, KMER, 0.05, 0)   # k = 0: nothing runs
    assert off0.tolist() == [0] * (n + 1) and len(nbrs0) == 0 and st["path"] == 0 and st["join_attempts"] == 0 and st["edges"] == 0
    got = ctx.knn_rows(idx, 0, KMER, 0.05, 65)   # one more than a wave has lanes
    check(got, hits, n, 65, 0)
    assert got[2]["path"] == 2 and got[2]["borderline"] == 0 and got[2]["max_degree"] == 0
    device = ctx.knn_rows(idx, 0, KMER, 0.05, 64)
    check(device, hits, n, 64, 0)
    assert device[2]["path"] == 1
    monkeypatch.setenv("RK_KNN_DEVICE", "0")
    host = ctx.knn_rows(idx, 0, KMER, 0.05, 64)
    check(host, hits, n, 64, 0)
    assert host[2]["path"] == 2 and np.array_equal(host[0], device[0])
    for f in capi.HIT_DTYPE.names:
        if f != "pad":
            assert np.array_equal(host[1][f], device[1][f]), f
    monkeypatch.delenv("RK_KNN_DEVICE")
    names, h, off, bits, wide, orc = collection("repeat")   # 64 genomes: k larger than N on the device
    got = ctx.knn_rows(device_index(ctx, h, off, bits), 0, KMER, 1.0, 64)
    want = check(got, orc.hits(0, 1.0), len(names), 64, 0)
    assert got[2]["path"] == 1 and len(names) <= 64 and max(len(one) for one in want) < 64


def test_knn_hits_over_dist_rows_equals_knn_rows(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for metric in (0, 1):
        off_d, nbrs, st = ctx.knn_rows(idx, metric, KMER, 0.05, 5)
        hits = ctx.dist_rows(idx, None, 1, metric, KMER, 0.05)[0]
        assert len(hits) == st["edges"] - st["borderline"] + st["borderline_kept"]
        off_h, host = capi.knn_hits(hits, n, 5, metric)
        assert np.array_equal(off_h, off_d)
        for f in capi.HIT_DTYPE.names:
            if f != "pad":
                assert np.array_equal(host[f], nbrs[f]), f


# ---- 11. nothing to select, and what is refused -------------------------------------------------------------------------
def test_empty_index_single_genome_and_no_pair(ctx):
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    off, nbrs, st = ctx.knn_rows(none, 0, KMER, 0.05, 3)
    assert off.tolist() == [0] and len(nbrs) == 0 and st["path"] == 0 and st["join_attempts"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for D in (0.05, 1.0):
        off, nbrs, st = ctx.knn_rows(one, 0, KMER, D, 3)
        assert off.tolist() == [0, 0] and len(nbrs) == 0 and st["edges"] == 0 and st["neighbours"] == 0 and st["max_degree"] == 0
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 0
    got = ctx.knn_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, 3)
    check(got, hits, 500, 3, 0)
    assert got[0].tolist() == [0] * 501 and got[2]["neighbours"] == 0 and got[2]["path"] == 1


def raw_call(ctx, idx, opts, n, k=3, off=True, nbrs=True, n_nbrs=True, stats=True):
    L = capi.lib()
    L.rk_knn_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p),
                              C.POINTER(C.c_uint64), C.POINTER(capi.KnnStats)]
    off_buf = np.zeros(n + 1, dtype=np.uint64)
    out, n_out, st = C.c_void_p(), C.c_uint64(), capi.KnnStats()
    rc = L.rk_knn_rows(ctx._h, idx._h, C.byref(opts), k, off_buf.ctypes.data if off else None, C.byref(out) if nbrs else None,
                       C.byref(n_out) if n_nbrs else None, C.byref(st) if stats else None)
    if nbrs:
        L.rk_free_host(out)
    return rc, int(n_out.value)


def test_arguments_that_are_refused(ctx):
    names, h, off, bits, wide, orc = collection("repeat")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for D in (1.5, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(capi.RkError) as e:
            ctx.knn_rows(idx, 0, KMER, D, 3)
        assert e.value.code == RK_ERR_ARG and "dense" in str(e.value)
    check(ctx.knn_rows(idx, 0, KMER, 1.0, 3), orc.hits(0, 1.0), n, 3, 0)   # the default -D 1.0 of alldist stays sparse
    assert raw_call(ctx, idx, capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1), n)[0] == RK_ERR_ARG   # triangle 0
    good = capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1)
    assert raw_call(ctx, idx, good, n, off=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, nbrs=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, n_nbrs=False)[0] == RK_ERR_ARG
    rc, n_nbrs = raw_call(ctx, idx, good, n, stats=False)   # stats is optional
    assert rc == 0 and n_nbrs > 0
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = orc.built
        ctx.knn_rows(ctx.index_import(postings, counts, 24, np.diff(off)), 0, KMER, 0.05, 3)
    assert e.value.code == RK_ERR_ARG


# ---- 12. the tool -------------------------------------------------------------------------------------------------------
def test_tool_knn_subcommand(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "ref.sketch")
    _, names, _, _ = ok.read_sketches32(os.path.join(GOLDEN, "dist", "ref.sketch"))
    assert len(set(names)) == len(names)
    n = len(names)
    number = {name: i for i, name in enumerate(names)}
    two = ["--gpus", "2", "--same-device"]
    for metric in (0, 1):
        lines = open(os.path.join(GOLDEN, "dist", "alldist_M%d_D0.3.ref.txt" % metric)).read().splitlines()
        hits, text = [], {}
        for line in lines:   # name[col] \t name[row] \t common|size0|size1 \t jorc \t dist  (the real reference's output)
            a, b, counts, jorc, dist = line.split("\t")
            hit = (number[b], number[a]) + tuple(int(x) for x in counts.split("|"))
            assert hit[0] < hit[1]
            hits.append(hit)
            text[hit[:2]] = (jorc, dist)
        for k in (1, 4):
            want = ""
            lists = kr.knn(hits, n, k, metric)
            for v in range(n):   # the genome first, then its neighbour; the sizes in that orientation
                for r in lists[v]:
                    sizes = (r[3], r[4]) if r[0] == v else (r[4], r[3])
                    want += "%s\t%s\t%d|%d|%d\t%s\t%s\n" % ((names[v], names[kr.other(r, v)], r[2]) + sizes + text[r[:2]])
            assert want.count("\n") > n // 2 and (k == 1 or any(r[1] == v and r[3] != r[4] for v in range(n) for r in lists[v]))
            for extra in (["--gpus", "1"], two):   # (the first run writes .dict / .index: the second takes the sharded build)
                out = tmp_path / ("k%d_%d_%d.txt" % (metric, k, len(extra)))
                p = subprocess.run([TOOL, "knn", "-i", "ref.sketch", "-D", "0.3", "-M", str(metric), "-N", str(k), "-o", out.name] + extra,
                                   cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                assert p.returncode == 0, p.stderr.decode()[-2000:]
                assert out.read_text() == want, (metric, k, extra)
    p = subprocess.run([TOOL, "knn", "-i", "ref.sketch", "-D", "0.3", "-o", "none.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"maxNeighbor must be >= 1" in p.stderr and not (tmp_path / "none.txt").exists()
    p = subprocess.run([TOOL, "knn", "-i", "ref.sketch", "-D", "1.5", "-N", "3", "-o", "dense.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"must not exceed 1.0" in p.stderr
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"knn -i" in p.stderr
