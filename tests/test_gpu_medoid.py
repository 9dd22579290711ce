"""rk_medoid_rows: the medoids and census of a clustering of the self join against tests/_medoid_ref.py (Python integers, exact rational
ratios) over the ORACLE's hit list, set up from tests/_selfjoin_cases.py (its Oracle, device_index and collections, built once per
session): degrees, sums and the two records of every genome, exactly -- the records byte for byte --, and the clusters rk_medoid_pick
makes of them.  Every case says from the reference or from the call's stats that it reached the edge it is about."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import _dbscan_ref as dr
import _medoid_ref as mr
from _selfjoin_cases import (KMER, TOOL, Oracle, both_overflows_collection, both_overflows_thresholds, bridge_collection, collection, csr, device_index,
                             identical, labels_of, permuted, tie_collection)
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth
from test_gpu_knn import cliques

pytestmark = pytest.mark.gpu
RK_ERR_ARG = -1
RK_MS_MEDOID = 11
NONE = mr.NONE
ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.POINTER(capi.MedoidGenomes), C.POINTER(capi.MedoidStats)]


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def records_of(want, by_pair):
    """the reference's hits (or None) of every genome as the library returns them: the oracle's record, pad 0; absent: row = col = NONE"""
    rec = np.zeros(len(want), dtype=capi.HIT_DTYPE)
    rec["row"] = rec["col"] = NONE
    for v, h in enumerate(want):
        if h is not None:
            rec[v] = by_pair[h[:2]]
            rec[v]["pad"] = 0
    return rec


def pairs_of(hits):
    return {(int(r["row"]), int(r["col"])): r for r in hits}


def check_arrays(got, hits, n, labels, metric, want=None):
    """(in_deg, out_deg, central, far_in, near_out) of a call or a fold against the reference over the oracle's hit list `hits`, then
    rk_medoid_pick over them against the reference's clusters; returns (the reference's arrays, its clusters)"""
    want = want or mr.genomes(mr.hit_tuples(hits), n, labels, metric)
    assert [a.dtype for a in got[:3]] == [np.uint32, np.uint32, np.uint64]
    for mine, ref, what in zip(got[:3], want[:3], ("in_deg", "out_deg", "central")):
        assert mine.tolist() == ref, what
    clusters = mr.pick(labels, want, metric)
    if got[3] is not None:
        by_pair = pairs_of(hits)
        assert got[3].dtype == got[4].dtype == capi.HIT_DTYPE
        assert got[3].tobytes() == records_of(want[3], by_pair).tobytes(), "far_in"   # byte for byte: the oracle's jorc and dist
        assert got[4].tobytes() == records_of(want[4], by_pair).tobytes(), "near_out"
        picked = capi.medoid_pick(labels, got[:5], metric)
        assert [int(x) for x in picked["label"]] == [c["label"] for c in clusters]
        for f in ("size", "medoid", "in_edges", "central"):
            assert picked[f].tolist() == [c[f] for c in clusters], f
        assert picked["weakest_in"].tobytes() == records_of([c["weakest_in"] for c in clusters], by_pair).tobytes()
        assert picked["nearest_out"].tobytes() == records_of([c["nearest_out"] for c in clusters], by_pair).tobytes()
    return want, clusters


def check(got, hits, n, labels, metric, shard_hits=None):
    """(in_deg, out_deg, central, far_in, near_out, stats) of one call (shard_hits: the records this call's row shard owns)"""
    mine = hits if shard_hits is None else shard_hits
    want, clusters = check_arrays(got, mine, n, labels, metric)
    st = got[5]
    assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
    assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(mine)   # the device consumed exactly the oracle's pairs
    assert st["inside"] == sum(want[0]) // 2 and st["leaving"] == sum(want[1]) // 2 and st["inside"] + st["leaving"] == len(mine)
    return want, clusters


# ---- 1. every pair at distance 0: q = 2^32, every extreme a tie ---------------------------------------------------------
def test_identical_sketches_under_three_labellings(ctx):
    h, off = csr(permuted(identical(300, 2), 12))
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 300 * 299 // 2 and np.all(hits["dist"] == 0.0)
    idx = device_index(ctx, h, off, 24)
    got = ctx.medoid_rows(idx, 0, KMER, 0.05, [0] * 300)
    want, clusters = check(got, hits, 300, [0] * 300, 0)
    assert got[2].tolist() == [299 << 32] * 300 and [c["medoid"] for c in clusters] == [0] and not got[1].any() and np.all(got[4]["row"] == NONE)
    assert [mr.other(want[3][v], v) for v in range(300)] == [1] + [0] * 299   # all ratios tie: the smallest neighbour
    parity = [v % 2 for v in range(300)]
    got = ctx.medoid_rows(idx, 0, KMER, 0.05, parity)
    want, clusters = check(got, hits, 300, parity, 0)
    assert got[2].tolist() == [149 << 32] * 300 and [c["medoid"] for c in clusters] == [0, 1] and got[1].tolist() == [150] * 300
    assert [mr.other(want[4][v], v) for v in range(300)] == [1, 0] * 150 and clusters[0]["nearest_out"][:2] == (0, 1)
    thirds = [7, 300 - 1, NONE] * 100   # two clusters named after genomes that are not their members, one third unlabelled
    got = ctx.medoid_rows(idx, 0, KMER, 0.05, thirds)
    want, clusters = check(got, hits, 300, thirds, 0)
    assert got[0].tolist() == [99, 99, 0] * 100 and got[1].tolist() == [200, 200, 299] * 100 and got[2].tolist() == [99 << 32, 99 << 32, 0] * 100
    assert [(c["label"], c["medoid"], c["size"], c["in_edges"]) for c in clusters] == [(7, 0, 100, 4950), (299, 1, 100, 4950)]


# ---- 2. degrees around the width of a wave ------------------------------------------------------------------------------
def test_cliques_around_the_width_of_a_wave(ctx):
    h, off, orc = cliques()
    n = len(off) - 1
    hits = orc.hits(0, 0.05)
    labels = labels_of(zip(hits["row"].tolist(), hits["col"].tolist()), n).tolist()
    idx = device_index(ctx, h, off, 24)
    got = ctx.medoid_rows(idx, 0, KMER, 0.05, labels)
    want, clusters = check(got, hits, n, labels, 0)
    assert sorted(set(want[0])) == [63, 64, 65, 128] and not any(want[1]) and got[5]["join_attempts"] == 1
    assert sorted(c["size"] for c in clusters) == [64, 65, 66, 129] and all(c["in_edges"] == c["size"] * (c["size"] - 1) // 2 for c in clusters)
    assert any(c["medoid"] != c["label"] for c in clusters) and len(set(want[2])) > 200   # random shares: many sums
    shifted = [(l + 1) % n for l in labels]   # the same partition under other names; then one clique cut in two: leaving records
    assert as_sums(ctx.medoid_rows(idx, 0, KMER, 0.05, shifted)) == as_sums(got)
    cut = [l if v % 2 or l != labels[0] else NONE for v, l in enumerate(labels)]
    got = ctx.medoid_rows(idx, 0, KMER, 0.05, cut)
    want, _ = check(got, hits, n, cut, 0)
    assert any(want[0]) and any(want[1])


def as_sums(got):
    return [a.tolist() for a in got[:3]] + [a.tobytes() for a in got[3:5]]


# ---- 3. contention: a star ----------------------------------------------------------------------------------------------
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
    first_leaf = 0 if centre else 1
    got = ctx.medoid_rows(idx, 0, KMER, 0.03, [5] * 3001)
    want, clusters = check(got, hits, 3001, [5] * 3001, 0)
    assert got[0][centre] == 3000 and int(got[2][centre]) == 3000 * ((60 << 32) // 140) and [c["medoid"] for c in clusters] == [centre]
    assert mr.other(want[3][centre], centre) == first_leaf and clusters[0]["in_edges"] == 3000   # 3,000 equal ratios at the hub: the smallest leaf
    alone = [NONE if v == centre else 5 for v in range(3001)]   # the hub unlabelled: every record is leaving
    got = ctx.medoid_rows(idx, 0, KMER, 0.03, alone)
    want, clusters = check(got, hits, 3001, alone, 0)
    assert got[1][centre] == 3000 and not got[0].any() and not got[2].any() and got[5]["leaving"] == 3000 and got[5]["inside"] == 0
    assert mr.other(want[4][centre], centre) == first_leaf and clusters[0]["medoid"] == first_leaf and clusters[0]["size"] == 3000
    assert clusters[0]["nearest_out"][:2] == tuple(sorted((centre, first_leaf))) and clusters[0]["weakest_in"] is None


# ---- 4. one ratio from different counts ---------------------------------------------------------------------------------
def test_equal_ratios_from_different_counts_go_to_the_smaller_index(ctx):
    h, off = tie_collection(3)   # six triangles A, B, C, one per assignment of the roles to ascending indices, and six plain pairs
    n = len(off) - 1
    hits = Oracle(h, off, 24).hits(0, 0.06)
    tuples = mr.hit_tuples(hits)
    idx = device_index(ctx, h, off, 24)
    whole = labels_of([t[:2] for t in tuples], n).tolist()
    got = ctx.medoid_rows(idx, 0, KMER, 0.06, whole)
    want, clusters = check(got, hits, n, whole, 0)
    seen = 0
    for k, roles in enumerate(itertools.permutations(range(3))):
        tri = list(range(5 * k, 5 * k + 3))
        mine = [t for t in tuples if t[0] in tri]
        assert len(mine) == 3 and {t[2] for t in mine} == {20, 25} and len({mr.ratio(t, 0) for t in mine}) == 1   # 25/75 = 20/60 = 20/60
        assert len({want[2][v] for v in tri}) == 1 and (25 << 32) // 75 == (20 << 32) // 60   # one q: three equal sums
        c = next(c for c in clusters if c["label"] == whole[tri[0]])
        assert c["medoid"] == tri[0] and c["weakest_in"][:2] == (tri[0], tri[1])
        assert [mr.other(want[3][v], v) for v in tri] == [tri[1], tri[0], tri[0]]
        seen += 1
    assert seen == 6
    # the same triangles with their second genome unlabelled: near_out of the other two ties between counts as well
    split = [NONE if v % 5 == 1 else l for v, l in enumerate(whole)]
    got = ctx.medoid_rows(idx, 0, KMER, 0.06, split)
    want, clusters = check(got, hits, n, split, 0)
    for k in range(6):
        a, b, c = 5 * k, 5 * k + 1, 5 * k + 2
        assert mr.other(want[4][b], b) == a and [mr.other(want[4][v], v) for v in (a, c)] == [b, b] and want[0][b] == 0 and want[1][b] == 2


# ---- 5. a pair exactly on the threshold, and one ulp either side --------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_bridge_on_the_threshold_and_one_ulp_either_side(ctx, metric):
    h, off = bridge_collection(2, 5)   # A, B, then a (70 of A's hashes) and b (70 of B's), who share 30 others: the bridge
    n = len(off) - 1
    a, b = n - 2, n - 1
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    labels = labels_of([t[:2] for t in mr.hit_tuples(orc.hits(metric, 0.03))], n).tolist()   # {A, a} and {B, b}
    assert len(set(labels)) == 2 and labels[a] != labels[b]
    for D, bridged in ((float(np.nextafter(d0, 0.0)), False), (d0, False), (float(np.nextafter(d0, 1.0)), True)):   # strict <
        hits = orc.hits(metric, D)
        assert len(hits) == 2 + int(bridged)
        got = ctx.medoid_rows(idx, metric, KMER, D, labels)
        want, clusters = check(got, hits, n, labels, metric)
        st = got[5]
        assert st["borderline"] >= 1 and st["borderline_kept"] == int(bridged) and st["leaving"] == int(bridged) and st["inside"] == 2
        assert [want[4][v] is not None for v in range(n)] == [False, False, bridged, bridged]   # near_out of a and b appears with the bridge
        assert all((c["nearest_out"] is not None) == bridged for c in clusters)
        if bridged:
            assert want[4][a][:2] == want[4][b][:2] == (a, b) and got[4]["dist"][a] == d0


# ---- 6. both overflows ---------------------------------------------------------------------------------------------------
def test_borderline_records_behind_both_overflows(ctx, monkeypatch):
    h, off = both_overflows_collection()
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    (D_above, _, _), _ = both_overflows_thresholds()
    above = orc.hits(0, D_above)
    labels = labels_of(zip(above["row"].tolist(), above["col"].tolist()), 420).tolist()   # the clique and ten clusters of two
    assert sorted(np.bincount(labels)[np.bincount(labels) > 0].tolist()) == [2] * 10 + [400]
    for D, n_hits, kept in both_overflows_thresholds():
        hits = orc.hits(0, D)
        assert len(hits) == n_hits > 65536
        got = ctx.medoid_rows(idx, 0, KMER, D, labels)
        want, clusters = check(got, hits, 420, labels, 0)
        st = got[5]
        assert st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        # one ulp above: the ten pairs are inside their clusters of two; on the distance itself: unreported
        small = [c for c in clusters if c["size"] == 2]
        assert len(small) == 10 and all(c["in_edges"] == (1 if kept else 0) and (c["weakest_in"] is not None) == bool(kept) for c in small)
        assert st["inside"] == 79800 + kept and st["leaving"] == 0
        assert sorted(got[0].tolist()) == [1 if kept else 0] * 20 + [399] * 400


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
    labels = orc.labels(metric, 0.02, kmer)[0].tolist()   # the clades frayed at 0.02, looked at within 0.05
    hits = orc.hits(metric, 0.05, kmer)
    got = ctx.medoid_rows(idx, metric, kmer, 0.05, labels)
    want, clusters = check(got, hits, n, labels, metric)
    st = got[5]
    expected = {"near": (4945, 455, 102), "wide": (6310, 440, 130), "repeat": (258, 18, 0)}.get(which)
    moved = sum(c["medoid"] != c["label"] for c in clusters)
    assert st["inside"] > 0 and st["leaving"] > 0 and (moved > 0) == (which != "repeat")
    if expected:
        assert (st["inside"], st["leaving"], moved) == expected
    else:
        assert 17498 <= st["inside"] <= 17731 and 1369 <= st["leaving"] <= 1562 and moved >= 379
    # oracles inside the project
    deg = ctx.dbscan_rows(idx, metric, kmer, 0.05, 1)[3]
    assert np.array_equal(got[0] + got[1], deg)
    off1, nearest, _ = ctx.knn_rows(idx, metric, kmer, 0.05, 1)
    for own in (list(range(n)), [NONE] * n):   # every genome its own cluster, or none labelled: every record is leaving
        lone = ctx.medoid_rows(idx, metric, kmer, 0.05, own)
        assert not lone[0].any() and not lone[2].any() and np.array_equal(lone[1], deg) and np.all(lone[3]["row"] == NONE)
        assert lone[4][lone[4]["row"] != NONE].tobytes() == nearest.tobytes() and np.array_equal(lone[4]["row"] != NONE, np.diff(off1) == 1)
    one = ctx.medoid_rows(idx, metric, kmer, 0.05, [0] * n)   # one cluster: nothing leaves
    assert not one[1].any() and np.all(one[4]["row"] == NONE) and np.array_equal(one[0], deg) and one[5]["leaving"] == 0


# ---- 8. row shards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [2, 3])
def test_row_shards_fold_to_the_whole(ctx, step):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    labels = orc.labels(0, 0.02)[0].tolist()
    hits = orc.hits(0, 0.05)
    whole = ctx.medoid_rows(idx, 0, KMER, 0.05, labels)
    folded, consumed = None, 0
    owner = idx.shard_of(hits, step, 32)
    for first in range(step):
        part = ctx.medoid_rows(idx, 0, KMER, 0.05, labels, row_first=first, row_step=step, row_block=32)
        own = hits[owner == first]
        check(part, hits, n, labels, 0, shard_hits=own)
        assert 0 < len(own) < len(hits)
        consumed += len(own)
        folded = part[:5] if folded is None else capi.medoid_merge(folded, part[:5], n, 0)
    assert consumed == len(hits) and as_sums(folded) == as_sums(whole)
    check_arrays(folded, hits, n, labels, 0)


def test_join_only_indexes_of_a_sharded_build_fold_to_the_whole(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=S))
    n = len(names)
    orc = Oracle(h, off, 20)
    hits = orc.hits(0, 0.1)
    labels = [NONE if v % 7 == 0 else l for v, l in enumerate(orc.labels(0, 0.04)[0].tolist())]   # (whole clades at 0.04: the unlabelled ones leave)
    assert len(hits) > 1000
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.medoid_rows(parts[0], 0, KMER, 0.1, labels)
    assert e.value.code == RK_ERR_ARG
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    folded, consumed = None, 0
    for d in range(S):   # the shards played in turn
        recv = torch.cat([bufs[r][12 * sum(sent[r][:d]): 12 * sum(sent[r][:d + 1])] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        j = ctx.index_join_shard(parts[d], recv.data_ptr(), sum(sent[r][d] for r in range(S)))
        part = ctx.medoid_rows(j, 0, KMER, 0.1, labels)
        assert part[5]["edges"] > 0
        consumed += part[5]["edges"] - part[5]["borderline"] + part[5]["borderline_kept"]
        folded = part[:5] if folded is None else capi.medoid_merge(folded, part[:5], n, 0)
        del j
    assert consumed == len(hits)
    want, _ = check_arrays(folded, hits, n, labels, 0)
    assert any(want[0]) and any(want[1])
    del parts, sk


# ---- 9. the host leg, and a call without records ------------------------------------------------------------------------
def test_host_leg_and_a_call_without_records(ctx, monkeypatch):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for metric in (0, 1):
        labels = orc.labels(metric, 0.02)[0].tolist()
        hits = orc.hits(metric, 0.05)
        device = ctx.medoid_rows(idx, metric, KMER, 0.05, labels)
        check(device, hits, n, labels, metric)
        assert device[5]["join_attempts"] == 1
        monkeypatch.setenv("RK_MEDOID_DEVICE", "0")
        host = ctx.medoid_rows(idx, metric, KMER, 0.05, labels)
        monkeypatch.delenv("RK_MEDOID_DEVICE")
        check(host, hits, n, labels, metric)
        assert host[5]["join_attempts"] == 0 and host[5]["edges"] == len(hits) and as_sums(host) == as_sums(device)
        ctx.set_timing(True)   # the call's timing slot: sums sweep through gather on the device leg, 0 on the host leg
        ctx.medoid_rows(idx, metric, KMER, 0.05, labels)
        assert ctx.last_ms(RK_MS_MEDOID) > 0.0
        monkeypatch.setenv("RK_MEDOID_DEVICE", "0")
        ctx.medoid_rows(idx, metric, KMER, 0.05, labels)
        monkeypatch.delenv("RK_MEDOID_DEVICE")
        assert ctx.last_ms(RK_MS_MEDOID) == 0.0
        ctx.set_timing(False)
        rows = ctx.dist_rows(idx, None, 1, metric, KMER, 0.05)[0]   # the host rule over the join's own hit list
        assert as_sums(capi.medoid_hits(rows, n, labels, metric)) == as_sums(device)
        bare = ctx.medoid_rows(idx, metric, KMER, 0.05, labels, records=False)
        assert bare[3] is None and bare[4] is None and [a.tolist() for a in bare[:3]] == as_sums(device)[:3]
        assert {k: v for k, v in bare[5].items()} == device[5]
        # the record arrays of a caller who asks for none of them stay as they were; one of the two alone is served
        L = capi.lib()
        L.rk_medoid_rows.argtypes = ROWS_ARGTYPES
        arrays = capi._medoid_arrays(n)
        arrays[3]["row"] = arrays[4]["row"] = 77
        lab = np.array(labels, dtype=np.uint32)
        opts = capi.DistOpts(1, metric, KMER, 0, 0.05, 0, 1)
        g = capi.MedoidGenomes(arrays[0].ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data, None, arrays[4].ctypes.data)
        assert L.rk_medoid_rows(ctx._h, idx._h, C.byref(opts), lab.ctypes.data, C.byref(g), None) == 0   # stats are optional
        assert np.all(arrays[3]["row"] == 77) and arrays[4].tobytes() == device[4].tobytes() and arrays[2].tolist() == device[2].tolist()


# ---- 10. nothing to sum, and what is refused ------------------------------------------------------------------------------
def test_empty_index_single_genome_and_no_pair(ctx):
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    got = ctx.medoid_rows(none, 0, KMER, 0.05, [])
    assert len(got[0]) == 0 and got[5]["join_attempts"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for label in (0, NONE):
        got = ctx.medoid_rows(one, 0, KMER, 0.05, [label])
        assert got[0].tolist() == got[1].tolist() == got[2].tolist() == [0] and got[3]["row"].tolist() == [NONE] and got[5]["edges"] == 0
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 0
    got = ctx.medoid_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, [v // 2 for v in range(500)])
    _, clusters = check(got, hits, 500, [v // 2 for v in range(500)], 0)
    assert got[5]["join_attempts"] == 1 and [c["medoid"] for c in clusters] == list(range(0, 500, 2))   # ties in central: the smaller index


def raw_call(ctx, idx, opts, n, labels, skip=None, with_out=True):
    L = capi.lib()
    L.rk_medoid_rows.argtypes = ROWS_ARGTYPES
    arrays = [np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint64), np.zeros(n, dtype=capi.HIT_DTYPE),
              np.zeros(n, dtype=capi.HIT_DTYPE)]
    arrays[3]["row"] = arrays[4]["row"] = 77
    g = capi.MedoidGenomes(*[None if k == skip else a.ctypes.data for k, a in enumerate(arrays)])
    st = capi.MedoidStats()
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    rc = L.rk_medoid_rows(ctx._h, idx._h, C.byref(opts), None if lab is None else lab.ctypes.data, C.byref(g) if with_out else None, C.byref(st))
    clean = all(np.all(a == 77) for a in arrays[:3]) and all(np.all(a["row"] == 77) and not a["common"].any() for a in arrays[3:])
    return rc, clean


def test_arguments_that_are_refused(ctx):
    names, h, off, bits, wide, orc = collection("repeat")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    labels = [0] * n
    for D in (1.5, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(capi.RkError) as e:
            ctx.medoid_rows(idx, 0, KMER, D, labels)
        assert e.value.code == RK_ERR_ARG and "dense" in str(e.value)
    check(ctx.medoid_rows(idx, 0, KMER, 1.0, labels), orc.hits(0, 1.0), n, labels, 0)   # the default -D 1.0 of alldist stays sparse
    good = capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    assert raw_call(ctx, idx, capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1), n, labels) == (RK_ERR_ARG, True) and b"triangle" in last()
    assert raw_call(ctx, idx, capi.DistOpts(1, 0, KMER, 0, 1.5, 0, 1), n, labels) == (RK_ERR_ARG, True) and b"dense" in last()
    for wrong in (n, n + 7, 0xFFFFFFFE):   # neither below N nor NONE
        assert raw_call(ctx, idx, good, n, labels[:-1] + [wrong]) == (RK_ERR_ARG, True) and b"label" in last()
    assert raw_call(ctx, idx, good, n, None) == (RK_ERR_ARG, True) and b"labels" in last()
    assert raw_call(ctx, idx, good, n, labels, with_out=False) == (RK_ERR_ARG, True)
    for skip in (0, 1, 2):   # the three sums are required
        assert raw_call(ctx, idx, good, n, labels, skip=skip) == (RK_ERR_ARG, True)
    for skip in (3, 4):      # each record array is optional
        rc, clean = raw_call(ctx, idx, good, n, labels, skip=skip)
        assert rc == 0 and not clean
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = orc.built
        ctx.medoid_rows(ctx.index_import(postings, counts, 24, np.diff(off)), 0, KMER, 0.05, labels)
    assert e.value.code == RK_ERR_ARG
    # a record outside 0 < common <= u: two copies of a sketch that lists every hash twice share 4 |S| counts
    twice = np.repeat(np.unique(np.random.default_rng(5).integers(0, 1 << 24, size=60))[:50], 2).astype(np.uint32)
    h2, off2 = csr([twice, twice, np.sort(twice[::2] ^ 1)])
    with pytest.raises(capi.RkError) as e:
        ctx.medoid_rows(device_index(ctx, h2, off2, 24), 1, KMER, 0.05, [0, 0, 0])
    assert e.value.code == -6 and "0 < common <= u" in str(e.value)


# ---- 11. the tool -------------------------------------------------------------------------------------------------------
def run_tool(tmp_path, args):
    return subprocess.run([TOOL, "medoid", "-i", "near.sketch"] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_medoid_subcommand(tmp_path):
    names, h, off, bits, wide, orc = collection("near")
    assert bits == 24 and len(set(names)) == len(names)
    synth.write_sketch_file(str(tmp_path / "near.sketch"), 10, 6, 4, names, h, off)   # 4 * (10 - 4) = 24 bits, k = 20
    n = len(names)

    def texts(labels, metric, D):
        hits = orc.hits(metric, D)
        g = mr.genomes(mr.hit_tuples(hits), n, labels, metric)
        return mr.render(names, labels, g, mr.pick(labels, g, metric), {p: float(r["dist"]) for p, r in pairs_of(hits).items()})
    # --labels FILE: the clades frayed at 0.02, every tenth genome unlabelled, looked at within 0.05
    frayed = [NONE if v % 10 == 3 else l for v, l in enumerate(orc.labels(0, 0.02)[0].tolist())]
    (tmp_path / "labels.txt").write_text("".join("-\n" if l == NONE else "%d\n" % l for l in frayed))
    out, census = texts(frayed, 0, 0.05)
    assert "\tnone\t" in out and "\tmember\t" in out and "\t-\t-\n" in out and "\t-\t-\t-\t" in census
    for extra, name in (([], "l1"), (["--gpus", "2", "--same-device"], "l2")):
        p = run_tool(tmp_path, ["-D", "0.05", "--labels", "labels.txt", "-o", name + ".txt", "--census", name + ".census"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert (tmp_path / (name + ".txt")).read_text() == out and (tmp_path / (name + ".census")).read_text() == census, name
    # --by cluster (the default), one and two GPUs, under containment
    single = orc.labels(1, 0.02)[0].tolist()
    out, census = texts(single, 1, 0.02)
    for extra, name in ((["--by", "cluster"], "c1"), (["--gpus", "2", "--same-device"], "c2")):
        p = run_tool(tmp_path, ["-D", "0.02", "-M", "1", "-o", name + ".txt", "--census", name + ".census"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert (tmp_path / (name + ".txt")).read_text() == out and (tmp_path / (name + ".census")).read_text() == census, name
    # --by dbscan -m 5: noise is unlabelled, a border genome's other core neighbours are leaving records
    dens = dr.dbscan(dr.hit_tuples(orc.hits(0, 0.02)), n, 5, 0)
    assert {0, 1, 2} == set(dens[1])
    out, census = texts(dens[0], 0, 0.02)
    p = run_tool(tmp_path, ["-D", "0.02", "--by", "dbscan", "-m", "5", "-o", "d.txt", "--census", "d.census"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert (tmp_path / "d.txt").read_text() == out and (tmp_path / "d.census").read_text() == census and "\tnone\t" in out
    # what dies, before a file is written
    p = run_tool(tmp_path, ["-D", "0.05", "--by", "greedy", "--gpus", "2", "-o", "g2.txt"])
    assert p.returncode != 0 and b"runs on one GPU" in p.stderr and not (tmp_path / "g2.txt").exists()
    p = run_tool(tmp_path, ["-D", "0.05", "--by", "dbscan", "-o", "d0.txt"])
    assert p.returncode != 0 and b"minPts must be >= 1" in p.stderr and not (tmp_path / "d0.txt").exists()
    (tmp_path / "short.txt").write_text("0\n" * (n - 1))
    (tmp_path / "long.txt").write_text("0\n" * (n + 1))
    (tmp_path / "big.txt").write_text("0\n" * (n - 1) + "%d\n" % n)
    (tmp_path / "word.txt").write_text("0\n" * (n - 1) + "x\n")
    for name in ("short", "long", "big", "word"):
        p = run_tool(tmp_path, ["-D", "0.05", "--labels", name + ".txt", "-o", name + ".out"])
        assert p.returncode != 0 and b"command_medoid()" in p.stderr and not (tmp_path / (name + ".out")).exists(), name
    p = run_tool(tmp_path, ["-D", "0.05", "--by", "greedy", "-o", "g1.txt"])   # a representative and its members: the medoid need not be it
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert len((tmp_path / "g1.txt").read_text().splitlines()) == n
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"medoid -i" in p.stderr and b" mreach medoid " in p.stderr
