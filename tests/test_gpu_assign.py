"""rk_assign_rows: the placement of query genomes into a labelled collection against tests/_assign_ref.py (Python integers, exact rational
ratios) over the ORACLE's hit list of the query join (index_dist32/64 with triangle = 0), set up from tests/_selfjoin_cases.py (its Oracle,
device_index and collections, built once per session): labels, the three counts and both records of every query, exactly -- the
records byte for byte.  Every case says from the oracle's list or from the call's stats that it reached the edge it is about."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _assign_ref as ar
import _dbscan_ref as dr
from _selfjoin_cases import KMER, TOOL, Oracle, collection, csr, device_index, identical
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6
RK_MS_ASSIGN = 12
NONE = ar.NONE
ROWS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.POINTER(capi.AssignQueries), C.POINTER(capi.AssignStats)]


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def query_hits(orc, qh, qoff, metric, D, kmer=KMER):
    """the oracle's hit list of the queries against the collection of `orc`: triangle = 0, dist <= D"""
    if orc.wide:
        uhash, ucount, postings = orc.built
        return ok.index_dist64(uhash, ucount, postings, orc.sizes, qh, qoff, 0, metric, kmer, D, threads=4)[0]
    postings, counts = orc.built
    return ok.index_dist32(counts, orc.bits, postings, orc.sizes, qh, qoff, 0, metric, kmer, D, threads=4)[0]


def device_queries(ctx, qh, qoff, wide=False):
    return ctx.sketches_from_host64(qh, qoff) if wide else ctx.sketches_from_host(qh, qoff)


def pairs_of(hits):
    return {(int(r["row"]), int(r["col"])): r for r in hits}


def records_of(want, by_pair):
    """the reference's hits (or None) of every query as the library returns them: the oracle's record, pad 0; absent: row = col = NONE"""
    rec = np.zeros(len(want), dtype=capi.HIT_DTYPE)
    rec["row"] = rec["col"] = NONE
    for v, h in enumerate(want):
        if h is not None:
            rec[v] = by_pair[h[:2]]
            rec[v]["pad"] = 0
    return rec


def check(got, hits, n_query, n_ref, labels, metric, stats=True):
    """(label, n_within, n_labelled, n_same, nearest, runner_up, stats) of one whole call against the reference over the oracle's list"""
    want = ar.assign(ar.hit_tuples(hits), n_query, n_ref, [int(l) for l in labels], metric)
    for mine, ref, what in zip(got[:4], want[:4], ("label", "n_within", "n_labelled", "n_same")):
        assert mine.dtype == np.uint32 and mine.tolist() == ref, what
    if got[4] is not None:
        by_pair = pairs_of(hits)
        assert got[4].dtype == got[5].dtype == capi.HIT_DTYPE
        assert got[4].tobytes() == records_of(want[4], by_pair).tobytes(), "nearest"   # byte for byte: the oracle's jorc and dist
        assert got[5].tobytes() == records_of(want[5], by_pair).tobytes(), "runner_up"
    if stats:
        st = got[6]
        assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
        assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(hits)   # the device consumed exactly the oracle's records
        assert st["placed"] == sum(l != NONE for l in want[0]) and st["novel"] == n_query - st["placed"]
        assert st["ambiguous"] == sum(h is not None for h in want[5])
    return want


def as_bytes(got):
    return [a.tolist() for a in got[:4]] + [None if a is None else a.tobytes() for a in got[4:6]]


def perturbed(h, off, picks, seed, bits, fresh=0.1):
    """queries: the sketches `picks` of a collection with a tenth of their hashes replaced by fresh values (a new strain)"""
    rng = np.random.default_rng(seed)
    parts = []
    for g in picks:
        mine = h[int(off[g]): int(off[g + 1])].copy()
        swap = rng.random(len(mine)) < fresh
        mine[swap] = rng.integers(0, 1 << bits, size=int(swap.sum()), dtype=np.uint64).astype(h.dtype)
        parts.append(np.unique(mine))
    return csr(parts, h.dtype)


_strains = {}


def strains(which):
    """(qh, qoff) of the queries of a named collection: every 7th genome perturbed, then two unrelated sketches and an empty one"""
    if which not in _strains:
        names, h, off, bits, wide, orc = collection(which)
        qh, qoff = perturbed(h, off, range(0, len(names), 7), 90 + len(names), bits)
        rng = np.random.default_rng(91)
        extra = [np.unique(rng.integers(0, 1 << bits, size=120, dtype=np.uint64)).astype(h.dtype) for _ in range(2)] + [np.zeros(0, dtype=h.dtype)]
        eh, eoff = csr(extra, h.dtype)
        _strains[which] = (np.concatenate([qh, eh]), np.concatenate([qoff, qoff[-1] + eoff[1:]]))
    return _strains[which]


# ---- 1. one ratio from different counts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_equal_ratios_from_different_counts_go_to_the_smaller_reference(ctx, metric):
    """The query A of 50 hashes shares 25 with B of 50 and 20 with C of 30 (metric 0: 25/75 = 20/60) or of 40 (metric 1: 25/50 = 20/40):
    B and C in different clusters, under both index orders of the pair -- the smaller index wins, the other is the runner-up"""
    rng = np.random.default_rng(40 + metric)
    pool = np.unique(rng.integers(0, 1 << 24, size=400)).astype(np.uint32)
    rng.shuffle(pool)
    abc, ab, ac, bc, a_own, b_own, c_own, other = np.split(pool[:195], [10, 25, 35, 45, 60, 75, 85])
    A = np.sort(np.concatenate([abc, ab, ac, a_own]))
    B = np.sort(np.concatenate([abc, ab, bc, b_own]))
    Cc = np.sort(np.concatenate([abc, ac, bc] + ([c_own] if metric else [])))
    qh, qoff = csr([A])
    for refs, common in (([B, Cc, np.sort(other)], (25, 20)), ([Cc, B, np.sort(other)], (20, 25))):
        h, off = csr(refs)
        orc = Oracle(h, off, 24)
        hits = query_hits(orc, qh, qoff, metric, 0.06)
        assert hits["col"].tolist() == [0, 1] and tuple(hits["common"].tolist()) == common and hits["dist"][0] == hits["dist"][1]
        assert len({ar.ratio(t, metric) for t in ar.hit_tuples(hits)}) == 1
        got = ctx.assign_rows(device_index(ctx, h, off, 24), device_queries(ctx, qh, qoff), metric, KMER, 0.06, [2, 1, 1])
        check(got, hits, 1, 3, [2, 1, 1], metric)
        assert got[0].tolist() == [2] and got[4]["col"].tolist() == [0] and got[5]["col"].tolist() == [1] and got[3].tolist() == [1]


# ---- 2. the threshold is <= ---------------------------------------------------------------------------------------------------
def threshold_case():
    """references: X of 100 hashes (cluster 0), Y (cluster 1), Z (cluster 2).  Queries: p shares 80 of its 100 hashes with X and nothing
    else; r shares 95 with Z and 80 with Y; s shares nothing."""
    rng = np.random.default_rng(44)
    pool = np.unique(rng.integers(0, 1 << 24, size=900)).astype(np.uint32)
    rng.shuffle(pool)
    X, Y, Z = pool[:100], pool[100:200], pool[200:300]
    p = np.concatenate([X[:80], pool[300:320]])
    r = np.concatenate([Z[:95], Y[:80], pool[320:345]])   # 200 hashes: 95 with Z (jaccard 95/205), 80 with Y (80/220)
    s = pool[400:500]
    return csr([np.sort(x) for x in (X, Y, Z)]), csr([np.sort(x) for x in (p, r, s)])


@pytest.mark.parametrize("metric", [0, 1])
def test_a_record_on_the_threshold_is_kept_and_decides(ctx, metric):
    """dist <= D.  A record ON the threshold is the farthest one the graph admits, so it cannot be nearer than a record the device decides;
    what it can do is be a query's only labelled record (novel or placed) or its only record of another cluster (runner-up or none)."""
    (h, off), (qh, qoff) = threshold_case()
    orc = Oracle(h, off, 24)
    idx, qs = device_index(ctx, h, off, 24), device_queries(ctx, qh, qoff)
    labels = [0, 1, 2]
    _, d0 = ok.distance(80, 100, 100, metric, KMER)       # p - X
    _, d1 = ok.distance(80, 100, 200, metric, KMER)       # r - Y
    assert d0 < d1 if metric == 0 else d0 == d1
    for D, p_placed in ((float(np.nextafter(d0, 0.0)), False), (d0, True), (float(np.nextafter(d0, 1.0)), True)):
        hits = query_hits(orc, qh, qoff, metric, D)
        got = ctx.assign_rows(idx, qs, metric, KMER, D, labels)
        want = check(got, hits, 3, 3, labels, metric)
        st = got[6]
        assert (want[0][0] == 0) == p_placed and want[0][2] == NONE and st["borderline"] >= 1
        if D == d0:
            assert st["borderline_kept"] >= 1 and got[4]["dist"][0] == D   # placed by a record the host decided
    for D, second in ((float(np.nextafter(d1, 0.0)), False), (d1, True), (float(np.nextafter(d1, 1.0)), True)):
        hits = query_hits(orc, qh, qoff, metric, D)
        got = ctx.assign_rows(idx, qs, metric, KMER, D, labels)
        want = check(got, hits, 3, 3, labels, metric)
        assert want[0][1] == 2 and (want[5][1] is not None) == second and got[6]["borderline"] >= 1 and got[6]["ambiguous"] == int(second)
        if second:
            assert want[5][1][1] == 1 and got[5]["dist"][1] == d1
    # with Z unlabelled the record on the threshold is r's only labelled one: the label itself flips
    for D, placed in ((float(np.nextafter(d1, 0.0)), False), (d1, True)):
        got = ctx.assign_rows(idx, qs, metric, KMER, D, [0, 1, NONE])
        want = check(got, query_hits(orc, qh, qoff, metric, D), 3, 3, [0, 1, NONE], metric)
        assert want[0][1] == (1 if placed else NONE) and want[1][1] == (2 if placed else 1)


# ---- 3. both overflows --------------------------------------------------------------------------------------------------------
def test_borderline_records_behind_both_overflows(ctx, monkeypatch):
    rng = np.random.default_rng(46)
    pool = np.unique(rng.integers(0, 1 << 24, size=2000)).astype(np.uint32)
    rng.shuffle(pool)
    one = np.sort(pool[:100])
    refs, queries = [one] * 400, [one] * 400
    for p in range(10):   # a pair shares 80 of 100
        mine = pool[100 + 120 * p: 220 + 120 * p]
        refs.append(np.sort(mine[:100]))
        queries.append(np.sort(mine[20:120]))
    order = np.random.default_rng(47).permutation(410)
    (h, off), (qh, qoff) = csr([refs[i] for i in order]), csr(queries)
    labels = [int(np.flatnonzero(order < 400)[0]) if order[i] < 400 else i for i in range(410)]   # the clique, and ten clusters of one
    orc = Oracle(h, off, 24)
    idx, qs = device_index(ctx, h, off, 24), device_queries(ctx, qh, qoff)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    _, d0 = ok.distance(80, 100, 100, 0, KMER)
    for D, kept in ((d0, 10), (float(np.nextafter(d0, 0.0)), 0)):
        hits = query_hits(orc, qh, qoff, 0, D)
        assert len(hits) == 160000 + kept > 65536
        got = ctx.assign_rows(idx, qs, 0, KMER, D, labels)
        check(got, hits, 410, 410, labels, 0)
        st = got[6]
        assert st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        assert st["placed"] == 400 + kept and st["novel"] == 10 - kept   # the borderline records decide ten placements
        assert got[1].tolist() == [400] * 400 + [1 if kept else 0] * 10
        monkeypatch.setenv("RK_ASSIGN_COMBINE", "0")   # 400 records per query: waves of one query and waves of two, lane by lane
        plain = ctx.assign_rows(idx, qs, 0, KMER, D, labels)
        monkeypatch.delenv("RK_ASSIGN_COMBINE")
        assert as_bytes(plain) == as_bytes(got) and plain[6] == got[6]


# ---- 4. contention, both ways -------------------------------------------------------------------------------------------------
def test_one_query_of_3000_references_and_3000_queries_of_one(ctx, monkeypatch):
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=140000)).astype(np.uint32)
    rng.shuffle(pool)
    hub, spare = pool[:100], pool[100:]
    leaves = [np.sort(np.concatenate([rng.choice(hub, size=60, replace=False), spare[40 * j: 40 * j + 40]])) for j in range(3000)]
    lone = np.sort(spare[130000:130100])
    (lh, loff), (hh, hoff) = csr(leaves), csr([np.sort(hub), lone])
    # every add and every minimum on one address: all 3,000 ratios tie (60/140)
    orc = Oracle(lh, loff, 24)
    hits = query_hits(orc, hh, hoff, 0, 0.03)
    assert len(hits) == 3000 and not hits["row"].any() and len(set(hits["dist"].tolist())) == 1
    labels = [1 - (v % 2) for v in range(3000)]
    got = ctx.assign_rows(device_index(ctx, lh, loff, 24), device_queries(ctx, hh, hoff), 0, KMER, 0.03, labels)
    check(got, hits, 2, 3000, labels, 0)
    assert got[0].tolist() == [1, NONE] and got[1].tolist() == [3000, 0] and got[3].tolist() == [1500, 0]
    assert got[4]["col"].tolist() == [0, NONE] and got[5]["col"].tolist() == [1, NONE]   # the smallest reference of either cluster
    monkeypatch.setenv("RK_ASSIGN_COMBINE", "0")   # every wave holds one query's records: the sweeps lane by lane give the same
    plain = ctx.assign_rows(device_index(ctx, lh, loff, 24), device_queries(ctx, hh, hoff), 0, KMER, 0.03, labels)
    monkeypatch.delenv("RK_ASSIGN_COMBINE")
    assert as_bytes(plain) == as_bytes(got) and plain[6] == got[6]
    # the other way round: 3,000 queries that see one reference each
    orc = Oracle(hh, hoff, 24)
    hits = query_hits(orc, lh, loff, 0, 0.03)
    assert len(hits) == 3000 and not hits["col"].any() and hits["row"].tolist() == list(range(3000))
    got = ctx.assign_rows(device_index(ctx, hh, hoff, 24), device_queries(ctx, lh, loff), 0, KMER, 0.03, [1, 0])
    check(got, hits, 3000, 2, [1, 0], 0)
    assert got[0].tolist() == [1] * 3000 and got[6]["placed"] == 3000 and got[6]["ambiguous"] == 0


# ---- 5. every query kernel path, both metrics, unlabelled references, one label, empty and disjoint queries ----------------
@pytest.mark.parametrize("which,metric", [("near", 0), ("near", 1), ("tiles", 0), ("tiles", 1), ("wide", 0), ("wide", 1)])
def test_perturbed_strains_of_every_collection(ctx, which, metric):
    names, h, off, bits, wide, orc = collection(which)
    kmer = 24 if wide else KMER
    n = len(names)
    qh, qoff = strains(which)
    nq = len(qoff) - 1
    idx, qs = device_index(ctx, h, off, bits, wide), device_queries(ctx, qh, qoff, wide)
    assert ctx.dist_kernel_name(idx, qs, 0, metric, kmer, 0.05).startswith("rk_distq_kernel<")
    hits = query_hits(orc, qh, qoff, metric, 0.05, kmer)
    labels = orc.labels(metric, 0.02, kmer)[0].tolist()   # the clades frayed at 0.02, looked at within 0.05
    got = ctx.assign_rows(idx, qs, metric, kmer, 0.05, labels)
    want = check(got, hits, nq, n, labels, metric)
    st = got[6]
    assert st["placed"] >= nq - 3 - 5 and st["ambiguous"] > 10 and st["sweeps"] == 5 and st["join_attempts"] == 1
    assert want[0][-3:] == [NONE] * 3 and want[1][-3:] == [0] * 3   # the unrelated and the empty queries: novel, no record
    # every third reference unlabelled: counted, never an anchor
    some = [NONE if v % 3 == 0 else l for v, l in enumerate(labels)]
    got = ctx.assign_rows(idx, qs, metric, kmer, 0.05, some)
    want = check(got, hits, nq, n, some, metric)
    first = {}
    for t in sorted(ar.hit_tuples(hits), key=lambda t: (t[0], -ar.ratio(t, metric), t[1])):
        first.setdefault(t[0], t)
    skipped = sum(some[first[q][1]] == NONE and want[4][q] is not None for q in first)
    assert skipped > 10 and sum(w > l for w, l in zip(want[1], want[2])) > 50   # the nearest overall is unlabelled: the anchor is the next one
    # none labelled: every query novel; one label: no runner-up, the support is every labelled record
    got = ctx.assign_rows(idx, qs, metric, kmer, 0.05, [NONE] * n)
    check(got, hits, nq, n, [NONE] * n, metric)
    assert np.all(got[0] == NONE) and got[6]["novel"] == nq and not got[2].any() and got[1].sum() == len(hits)
    got = ctx.assign_rows(idx, qs, metric, kmer, 0.05, [n - 1] * n)
    check(got, hits, nq, n, [n - 1] * n, metric)
    assert np.all(got[5]["row"] == NONE) and np.array_equal(got[3], got[2]) and np.array_equal(got[2], got[1]) and got[6]["ambiguous"] == 0


def test_kernel_paths_differ_between_the_collections(ctx):
    name = {}
    for which in ("near", "wide"):
        names, h, off, bits, wide, orc = collection(which)
        qh, qoff = strains(which)
        name[which] = ctx.dist_kernel_name(device_index(ctx, h, off, bits, wide), device_queries(ctx, qh, qoff, wide), 0, 0, 24 if wide else KMER, 0.05)
    assert name["near"] != name["wide"]   # another look-up at 36 bits


def test_no_query_and_no_reference(ctx):
    names, h, off, bits, wide, orc = collection("near")
    idx = device_index(ctx, h, off, bits)
    got = ctx.assign_rows(idx, device_queries(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64)), 0, KMER, 0.05, [0] * len(names))
    assert all(len(a) == 0 for a in got[:6]) and got[6]["join_attempts"] == 0 and got[6]["placed"] == got[6]["novel"] == 0
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 24)
    qh, qoff = strains("near")
    got = ctx.assign_rows(none, device_queries(ctx, qh, qoff), 0, KMER, 0.05, [])
    nq = len(qoff) - 1
    assert np.all(got[0] == NONE) and not got[1].any() and np.all(got[4]["row"] == NONE) and got[6]["novel"] == nq and got[6]["join_attempts"] == 0


# ---- 6. multisets are refused ---------------------------------------------------------------------------------------------------
def test_a_multiset_record_is_refused(ctx):
    names, h, off, bits, wide, orc = collection("repeat")   # its first sketch lists one hash twice
    qh, qoff = csr([h[int(off[g]): int(off[g + 1])] for g in range(4)])
    hits = query_hits(orc, qh, qoff, 1, 0.05)
    own = hits[(hits["row"] == 0) & (hits["col"] == 0)]
    assert len(own) == 1 and own["common"][0] > min(own["size0"][0], own["size1"][0])   # outside 0 < common <= u
    out = sentinel(4)
    with pytest.raises(capi.RkError) as e:
        ctx.assign_rows(device_index(ctx, h, off, bits), device_queries(ctx, qh, qoff), 1, KMER, 0.05, [0] * len(names), out=out)
    assert e.value.code == RK_ERR_UNSUPPORTED and "0 < common <= u" in str(e.value) and untouched(out)


# ---- 7. row shards ------------------------------------------------------------------------------------------------------------
def sentinel(q):
    out = tuple(np.full(q, 0xABABABAB, dtype=np.uint32) for _ in range(4)) + (np.zeros(q, dtype=capi.HIT_DTYPE), np.zeros(q, dtype=capi.HIT_DTYPE))
    out[4]["common"] = out[5]["common"] = 77
    return out


def untouched(out, rows=slice(None)):
    return all(np.all(a[rows] == 0xABABABAB) for a in out[:4]) and all(np.all(a["common"][rows] == 77) and not a["row"][rows].any() for a in out[4:])


@pytest.mark.parametrize("step,block", [(2, 1), (3, 1), (2, 32), (3, 32)])
def test_row_shards_write_their_rows_into_one_set_of_arrays(ctx, step, block):
    names, h, off, bits, wide, orc = collection("near")
    qh, qoff = strains("near")
    nq = len(qoff) - 1
    idx, qs = device_index(ctx, h, off, bits), device_queries(ctx, qh, qoff)
    labels = orc.labels(0, 0.02)[0].tolist()
    whole = ctx.assign_rows(idx, qs, 0, KMER, 0.05, labels)
    check(whole, query_hits(orc, qh, qoff, 0, 0.05), nq, len(names), labels, 0)
    owner = (np.arange(nq) // block) % step
    shared = sentinel(nq)
    placed = 0
    for first in range(step):
        mine = owner == first
        assert 0 < mine.sum() < nq
        alone = sentinel(nq)
        st = ctx.assign_rows(idx, qs, 0, KMER, 0.05, labels, row_first=first, row_step=step, row_block=block, out=alone)[6]
        assert untouched(alone, ~mine)   # the entries of unselected rows are not written
        assert all(np.array_equal(a[mine], w[mine]) for a, w in zip(alone, whole[:6]))
        assert st["placed"] + st["novel"] == mine.sum()
        placed += st["placed"]
        ctx.assign_rows(idx, qs, 0, KMER, 0.05, labels, row_first=first, row_step=step, row_block=block, out=shared)
    assert as_bytes(shared) == as_bytes(whole) and placed == whole[6]["placed"]   # the shards together are the whole: no merge


# ---- 8. without record arrays, the host leg -----------------------------------------------------------------------------------
def test_host_leg_and_a_call_without_records(ctx, monkeypatch):
    names, h, off, bits, wide, orc = collection("near")
    qh, qoff = strains("near")
    nq, n = len(qoff) - 1, len(names)
    idx, qs = device_index(ctx, h, off, bits), device_queries(ctx, qh, qoff)
    for metric in (0, 1):
        labels = [NONE if v % 5 == 0 else l for v, l in enumerate(orc.labels(metric, 0.02)[0].tolist())]
        hits = query_hits(orc, qh, qoff, metric, 0.05)
        device = ctx.assign_rows(idx, qs, metric, KMER, 0.05, labels)
        check(device, hits, nq, n, labels, metric)
        monkeypatch.setenv("RK_ASSIGN_DEVICE", "0")
        host = ctx.assign_rows(idx, qs, metric, KMER, 0.05, labels)
        shard = sentinel(nq)
        ctx.assign_rows(idx, qs, metric, KMER, 0.05, labels, row_first=1, row_step=2, row_block=3, out=shard)
        monkeypatch.delenv("RK_ASSIGN_DEVICE")
        check(host, hits, nq, n, labels, metric, stats=False)
        assert host[6]["join_attempts"] == 0 and host[6]["sweeps"] == 0 and host[6]["edges"] == len(hits) and as_bytes(host) == as_bytes(device)
        assert {k: host[6][k] for k in ("placed", "novel", "ambiguous")} == {k: device[6][k] for k in ("placed", "novel", "ambiguous")}
        mine = (np.arange(nq) // 3) % 2 == 1   # the host leg writes its rows alone as well
        assert untouched(shard, ~mine) and all(np.array_equal(a[mine], w[mine]) for a, w in zip(shard, device[:6]))
        ctx.set_timing(True)   # the call's timing slot: first sweep through gather on the device leg, 0 on the host leg
        ctx.assign_rows(idx, qs, metric, KMER, 0.05, labels)
        assert ctx.last_ms(RK_MS_ASSIGN) > 0.0
        monkeypatch.setenv("RK_ASSIGN_DEVICE", "0")
        ctx.assign_rows(idx, qs, metric, KMER, 0.05, labels)
        monkeypatch.delenv("RK_ASSIGN_DEVICE")
        assert ctx.last_ms(RK_MS_ASSIGN) == 0.0
        ctx.set_timing(False)
        rows = ctx.dist_rows(idx, qs, 0, metric, KMER, 0.05)[0]   # the host rule over the join's own hit list
        assert as_bytes(capi.assign_hits(rows, nq, n, labels, metric)) == as_bytes(device)
        bare = ctx.assign_rows(idx, qs, metric, KMER, 0.05, labels, records=False)
        assert bare[4] is None and bare[5] is None and as_bytes(bare)[:4] == as_bytes(device)[:4]
        assert bare[6]["sweeps"] == 3 and device[6]["sweeps"] == 5   # the runner-up's settle sweep and the gather did not run
        assert {k: v for k, v in bare[6].items() if k != "sweeps"} == {k: v for k, v in device[6].items() if k != "sweeps"}
        # one of the two record arrays alone is served, the other stays as it was; stats are optional
        L = capi.lib()
        L.rk_assign_rows.argtypes = ROWS_ARGTYPES
        arrays = sentinel(nq)
        lab = np.array(labels, dtype=np.uint32)
        opts = capi.DistOpts(0, metric, KMER, 0, 0.05, 0, 1)
        g = capi.AssignQueries(*[a.ctypes.data for a in arrays[:4]], None, arrays[5].ctypes.data)
        assert L.rk_assign_rows(ctx._h, idx._h, qs._h, C.byref(opts), lab.ctypes.data, C.byref(g), None) == 0
        assert np.all(arrays[4]["common"] == 77) and not arrays[4]["row"].any() and arrays[5].tobytes() == device[5].tobytes()
        assert arrays[0].tolist() == device[0].tolist()


# ---- 9. what is refused -------------------------------------------------------------------------------------------------------
def raw_call(ctx, idx, qs, opts, nq, labels, skip=None, with_out=True):
    L = capi.lib()
    L.rk_assign_rows.argtypes = ROWS_ARGTYPES
    arrays = sentinel(nq)
    g = capi.AssignQueries(*[None if k == skip else a.ctypes.data for k, a in enumerate(arrays)])
    st = capi.AssignStats()
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    rc = L.rk_assign_rows(ctx._h, idx._h, None if qs is None else qs._h, C.byref(opts), None if lab is None else lab.ctypes.data,
                          C.byref(g) if with_out else None, C.byref(st))
    return rc, untouched(arrays)


def test_arguments_that_are_refused(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    qh, qoff = strains("near")
    nq = len(qoff) - 1
    idx, qs = device_index(ctx, h, off, bits), device_queries(ctx, qh, qoff)
    labels = [0] * n
    for D in (1.0, 1.5):   # triangle = 0: the report is dense AT 1.0
        with pytest.raises(capi.RkError) as e:
            ctx.assign_rows(idx, qs, 0, KMER, D, labels)
        assert e.value.code == RK_ERR_ARG and "dense" in str(e.value)
    good = capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1)
    last = lambda: capi.lib().rk_last_error(ctx._h)   # noqa: E731
    assert raw_call(ctx, idx, qs, capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1), nq, labels) == (RK_ERR_ARG, True) and b"triangle" in last()
    assert raw_call(ctx, idx, None, good, nq, labels) == (RK_ERR_ARG, True) and b"queries is null" in last()
    assert raw_call(ctx, idx, qs, capi.DistOpts(0, 0, KMER, 0, 1.0, 0, 1), nq, labels) == (RK_ERR_ARG, True) and b"dense" in last()
    assert raw_call(ctx, idx, qs, capi.DistOpts(0, 0, 0, 0, 0.05, 0, 1), nq, labels) == (RK_ERR_ARG, True) and b"kmer_size" in last()
    assert raw_call(ctx, idx, qs, capi.DistOpts(0, 0, KMER, -1, 0.05, 0, 1), nq, labels) == (RK_ERR_ARG, True) and b"row_block" in last()
    for wrong in (n, n + 7, 0xFFFFFFFE):   # neither below N nor NONE
        assert raw_call(ctx, idx, qs, good, nq, labels[:-1] + [wrong]) == (RK_ERR_ARG, True) and b"label" in last()
    assert raw_call(ctx, idx, qs, good, nq, None) == (RK_ERR_ARG, True) and b"labels is null" in last()
    assert raw_call(ctx, idx, qs, good, nq, labels, with_out=False) == (RK_ERR_ARG, True) and b"out is null" in last()
    for skip in (0, 1, 2, 3):   # the label and the three counts are required
        assert raw_call(ctx, idx, qs, good, nq, labels, skip=skip) == (RK_ERR_ARG, True) and b"of out is null" in last()
    for skip in (4, 5):         # each record array is optional
        rc, clean = raw_call(ctx, idx, qs, good, nq, labels, skip=skip)
        assert rc == 0 and not clean
    # queries of the other hash width
    wnames, wh, woff, wbits, _, _ = collection("wide")
    wqs = device_queries(ctx, *strains("wide"), wide=True)
    assert raw_call(ctx, idx, wqs, good, wqs.count, labels) == (RK_ERR_ARG, True) and b"hash widths" in last()
    # an imported index answers explicit queries: no refusal
    postings, counts = orc.built
    imported = ctx.index_import(postings, counts, 24, np.diff(off))
    assert as_bytes(ctx.assign_rows(imported, qs, 0, KMER, 0.05, labels)) == as_bytes(ctx.assign_rows(idx, qs, 0, KMER, 0.05, labels))


def test_indexes_without_posting_lists_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    n = len(names)
    sk = ctx.sketches_from_host(h, off)
    qh, qoff = perturbed(h, off, range(0, n, 9), 54, 20)
    qs = device_queries(ctx, qh, qoff)
    nq = len(qoff) - 1
    good = capi.DistOpts(0, 0, KMER, 0, 0.1, 0, 1)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    assert raw_call(ctx, parts[0], qs, good, nq, [0] * n) == (RK_ERR_ARG, True)   # one hash range of a sharded build
    assert b"without posting lists" in capi.lib().rk_last_error(ctx._h)
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
    assert raw_call(ctx, j, qs, good, nq, [0] * n) == (RK_ERR_ARG, True)   # the join-only index: tile records of its rows, no lists
    assert b"without posting lists" in capi.lib().rk_last_error(ctx._h)
    del j, parts, sk


# ---- 10. the tool -------------------------------------------------------------------------------------------------------------
def run_tool(tmp_path, args):
    return subprocess.run([TOOL, "assign", "-r", "near.sketch", "-q", "strains.sketch"] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("metric", [0, 1])
def test_tool_assign_subcommand(tmp_path, metric):
    names, h, off, bits, wide, orc = collection("near")
    assert bits == 24 and len(set(names)) == len(names)
    qh, qoff = strains("near")
    nq, n = len(qoff) - 1, len(names)
    qnames = ["new/q%04d.fna" % q for q in range(nq)]
    synth.write_sketch_file(str(tmp_path / "near.sketch"), 10, 6, 4, names, h, off)   # 4 * (10 - 4) = 24 bits, k = 20
    synth.write_sketch_file(str(tmp_path / "strains.sketch"), 10, 6, 4, qnames, qh, qoff)
    M = ["-M", str(metric)]

    def texts(labels, D):
        hits = query_hits(orc, qh, qoff, metric, D)
        result = ar.assign(ar.hit_tuples(hits), nq, n, labels, metric)
        values = {p: (float(r["jorc"]), float(r["dist"])) for p, r in pairs_of(hits).items()}
        return ar.render(qnames, names, labels, result, values), ar.novel(qnames, result)
    # --labels FILE: the clades frayed at 0.02, every tenth reference unlabelled, looked at within 0.05
    frayed = [NONE if v % 10 == 3 else l for v, l in enumerate(orc.labels(metric, 0.02)[0].tolist())]
    (tmp_path / "labels.txt").write_text("".join("-\n" if l == NONE else "%d\n" % l for l in frayed))
    out, novel = texts(frayed, 0.05)
    assert "\t-\t-\n" in out and "\t-\t-\t-\t-\t-\t0\t0\t" in out and len(novel.splitlines()) >= 3 and out.count("\n") == nq
    assert sum(not line.endswith("\t-\t-") for line in out.splitlines()) > 10   # runner-ups
    for extra, name in (([], "l1"), (["--gpus", "2", "--same-device"], "l2")):
        p = run_tool(tmp_path, M + ["-D", "0.05", "--labels", "labels.txt", "-o", name + ".txt", "--novel", name + ".novel"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert (tmp_path / (name + ".txt")).read_text() == out and (tmp_path / (name + ".novel")).read_text() == novel, name
    # --by cluster (the default) is --labels with the single-linkage labels of the same -D; one and two GPUs
    single = orc.labels(metric, 0.02)[0].tolist()
    out, novel = texts(single, 0.02)
    (tmp_path / "single.txt").write_text("".join("%d\n" % l for l in single))
    for extra, name in ((["--by", "cluster"], "c1"), (["--gpus", "2", "--same-device"], "c2"), (["--labels", "single.txt"], "c3")):
        p = run_tool(tmp_path, M + ["-D", "0.02", "-o", name + ".txt", "--novel", name + ".novel"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert (tmp_path / (name + ".txt")).read_text() == out and (tmp_path / (name + ".novel")).read_text() == novel, name
    # --by dbscan -m 5: only the core references anchor a query
    dens = dr.dbscan(dr.hit_tuples(orc.hits(metric, 0.02)), n, 5, metric)
    assert {0, 1, 2} == set(dens[1])
    cores = [l if k == 2 else NONE for l, k in zip(dens[0], dens[1])]
    out, novel = texts(cores, 0.02)
    for extra, name in (([], "d1"), (["--gpus", "2", "--same-device"], "d2")):
        p = run_tool(tmp_path, M + ["-D", "0.02", "--by", "dbscan", "-m", "5", "-o", name + ".txt", "--novel", name + ".novel"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert (tmp_path / (name + ".txt")).read_text() == out and (tmp_path / (name + ".novel")).read_text() == novel, name
    if metric:
        return
    p = run_tool(tmp_path, ["-D", "0.05", "--by", "greedy", "-o", "g1.txt"])   # a representative's name is the cluster's
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert len((tmp_path / "g1.txt").read_text().splitlines()) == nq
    # what dies, before a file is written
    for D in ("1.0", "1.5"):
        p = run_tool(tmp_path, ["-D", D, "-o", "dense.txt"])
        assert p.returncode != 0 and b"must stay below 1.0" in p.stderr and b"dense" in p.stderr and not (tmp_path / "dense.txt").exists()
    p = run_tool(tmp_path, ["-o", "nod.txt"])
    assert p.returncode != 0 and b"needs -D" in p.stderr and not (tmp_path / "nod.txt").exists()
    p = run_tool(tmp_path, ["-D", "0.05", "--by", "dbscan", "-o", "d0.txt"])
    assert p.returncode != 0 and b"minPts must be >= 1" in p.stderr and not (tmp_path / "d0.txt").exists()
    p = run_tool(tmp_path, ["-D", "0.05", "--by", "cluster", "--labels", "labels.txt", "-o", "both.txt"])
    assert p.returncode != 0 and b"exclude each other" in p.stderr and not (tmp_path / "both.txt").exists()
    (tmp_path / "short.txt").write_text("0\n" * (n - 1))
    (tmp_path / "long.txt").write_text("0\n" * (n + 1))
    (tmp_path / "big.txt").write_text("0\n" * (n - 1) + "%d\n" % n)
    (tmp_path / "word.txt").write_text("0\n" * (n - 1) + "x\n")
    for name in ("short", "long", "big", "word"):
        p = run_tool(tmp_path, ["-D", "0.05", "--labels", name + ".txt", "-o", name + ".out"])
        assert p.returncode != 0 and b"command_assign()" in p.stderr and not (tmp_path / (name + ".out")).exists(), name
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"assign -r" in p.stderr and b" medoid assign dist " in p.stderr
