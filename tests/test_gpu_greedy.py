"""rk_greedy_rows: the greedy representatives of the self join against tests/_greedy_ref.py's sequential rule (exact rational
ratios) over the ORACLE's hit list, set up from tests/_selfjoin_cases.py (its Oracle, device_index and collections, built
once per session): rep, the exact link tuples, and jorc / dist of the links bit for bit.  Every case says from the call's
stats that it reached the edge it is about; the number of rounds is that of the reference's model of the rounds."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _greedy_ref as gr
from _selfjoin_cases import (KMER, TOOL, Oracle, borderline_overflow_collection, both_overflows_collection, both_overflows_thresholds,
                             collection, csr, device_index, hit_overflow_collection, identical, permuted, trio)
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu
RK_ERR_ARG, RK_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def check(got, hits, n, metric, priority=None, sizes=None):
    """(rep, links, stats) of one call against the oracle's hit list; returns the reference's (rep, links)"""
    rep, links, st = got
    tuples = gr.hit_tuples(hits)
    want_rep, want_links = gr.greedy(tuples, n, metric, priority, sizes)
    assert rep.dtype == np.uint32 and rep.tolist() == want_rep
    members = sorted(want_links)
    assert gr.hit_tuples(links) == [want_links[m] for m in members]
    value = {(int(r), int(c)): (float(j), float(d)) for r, c, j, d in zip(hits["row"], hits["col"], hits["jorc"], hits["dist"])}
    assert np.array_equal(links["jorc"], np.array([value[want_links[m][:2]][0] for m in members], dtype=np.float64))
    assert np.array_equal(links["dist"], np.array([value[want_links[m][:2]][1] for m in members], dtype=np.float64))
    assert np.all(links["row"] < links["col"])
    assert st["n_reps"] == n - len(members) == sum(want_rep[i] == i for i in range(n))
    assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
    assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(hits)   # the device consumed exactly the oracle's pairs
    assert st["rounds"] == gr.rounds(tuples, n, priority, sizes)[1]
    return want_rep, want_links


def path_parts(n, m, seed):
    """the path of test_path_of_2048_genomes: genome i + 1 keeps 50 .. 95 of genome i's m hashes (d <= 0.0347), the rest fresh"""
    rng = np.random.default_rng(seed)
    share = rng.integers(50, 96, size=n - 1)
    pool = np.unique(rng.integers(0, 1 << 24, size=70 * n))
    rng.shuffle(pool)
    assert len(pool) >= m + int((m - share).sum())
    parts, used = [pool[:m]], m
    for i in range(n - 1):
        fresh = m - int(share[i])
        parts.append(np.concatenate([rng.choice(parts[-1], size=int(share[i]), replace=False), pool[used: used + fresh]]))
        used += fresh
    return [np.sort(p) for p in parts]


# ---- 1. a path laid in priority order: one round after the other ----------------------------------------------------------
def test_path_laid_in_priority_order(ctx):
    n = 1024
    parts = path_parts(n, 100, 1)   # equal sizes: the priority order is the caller's order, which is the path's
    h, off = csr(parts)
    orc = Oracle(h, off, 24)
    hits = orc.hits(0, 0.05)
    got = ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    rep, links = check(got, hits, n, 0, sizes=orc.sizes)
    st = got[2]
    assert st["rounds"] >= 512 and st["join_attempts"] == 1 and st["border_attempts"] == 1
    # along the path: every member hangs on a representative a few steps back, and no two representatives are neighbours
    assert rep[0] == 0 and all(rep[i] <= i for i in range(n)) and not any(rep[i] == i and rep[i + 1] == i + 1 for i in range(n - 1))
    assert st["n_reps"] <= n // 2
    h2, off2 = csr(permuted(parts, 11))   # the same path in a shuffled order: many ends to start from
    orc2 = Oracle(h2, off2, 24)
    got2 = ctx.greedy_rows(device_index(ctx, h2, off2, 24), 0, KMER, 0.05)
    check(got2, orc2.hits(0, 0.05), n, 0, sizes=orc2.sizes)
    assert 2 <= got2[2]["rounds"] < st["rounds"]


# ---- 2. every pair at distance 0 ----------------------------------------------------------------------------------------
_identical_300 = {}


def identical_300():
    if not _identical_300:
        h, off = csr(permuted(identical(300, 2), 12))
        _identical_300["it"] = (h, off, Oracle(h, off, 24))
    return _identical_300["it"]


def test_identical_sketches_have_one_representative(ctx):
    h, off, orc = identical_300()
    hits = orc.hits(0, 0.05)
    assert len(hits) == 300 * 299 // 2 and np.all(hits["dist"] == 0.0)
    got = ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    check(got, hits, 300, 0, sizes=orc.sizes)
    rep, links, st = got
    assert np.all(rep == 0) and st["n_reps"] == 1 and st["edges"] == 44850 and st["rounds"] <= 3
    assert links["row"].tolist() == [0] * 299 and links["col"].tolist() == list(range(1, 300)) and np.all(links["dist"] == 0.0)


# ---- 3. one ratio from different counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_equal_ratio_from_different_counts(ctx, metric):
    # metric 0: the member's 30 hashes, 20 of them in a representative of 50 (20/60) and 25 in one of 70 (25/75); the two share the
    # forced 15: jaccard 15/105, Mash distance 0.069.  metric 1 (u = the smaller sketch): 16 in a representative of 24 (16/24) and
    # 20 in one of 70 (20/30); the two share the forced 6 of 24: AafD 0.069.  There the member is not the smallest sketch, so the
    # representatives come first by an explicit priority
    sizes, shares = ((50, 70, 30), (20, 25)) if metric == 0 else ((24, 70, 30), (16, 20))
    for roles in ((0, 1, 2), (1, 0, 2)):
        h, off = trio(3, sizes, shares, roles)
        orc = Oracle(h, off, 24)
        hits = orc.hits(metric, 0.05)
        tuples = gr.hit_tuples(hits)
        assert [t[:2] for t in tuples] == [(0, 2), (1, 2)]   # the two representatives are not adjacent
        assert gr.ratio(tuples[0], metric) == gr.ratio(tuples[1], metric) and tuples[0][2] != tuples[1][2]
        priority = None if metric == 0 else [0, 0, 1]
        got = ctx.greedy_rows(device_index(ctx, h, off, 24), metric, KMER, 0.05, priority)
        check(got, hits, 3, metric, priority, sizes=orc.sizes)
        assert got[0].tolist() == [0, 1, 0] and gr.hit_tuples(got[1]) == [tuples[0]] and got[2]["rounds"] == 2


# ---- 4. a nearer representative that comes later ------------------------------------------------------------------------
def test_a_nearer_later_representative_is_not_taken(ctx):
    # R1 (120 hashes) before M (100) before R2 (80) by size; M shares 50 with R1 (d 0.039) and 70 with R2 (d 0.011); R1 and R2 share
    # the forced 20 (d 0.08)
    for roles in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        h, off = trio(4, (120, 80, 100), (50, 70), roles)
        r1, r2, m = roles.index(0), roles.index(1), roles.index(2)
        orc = Oracle(h, off, 24)
        hits = orc.hits(0, 0.05)
        assert sorted(t[:2] for t in gr.hit_tuples(hits)) == sorted([tuple(sorted((r1, m))), tuple(sorted((r2, m)))])
        got = ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
        rep, links = check(got, hits, 3, 0, sizes=orc.sizes)
        assert rep[m] == r1 and rep[r1] == r1 and rep[r2] == r2
        assert gr.ratio(links[m], 0) < max(gr.ratio(t, 0) for t in gr.hit_tuples(hits))   # (the other record is the nearer one)


# ---- 5. the caller's priority -------------------------------------------------------------------------------------------
def test_custom_priority(ctx):
    h, off, orc = identical_300()
    priority = np.arange(299, -1, -1, dtype=np.uint32)
    got = ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05, priority)
    check(got, orc.hits(0, 0.05), 300, 0, priority)
    assert np.all(got[0] == 299) and got[2]["n_reps"] == 1
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    plain = ctx.greedy_rows(idx, 0, KMER, 0.05)
    check(plain, orc.hits(0, 0.05), n, 0, sizes=orc.sizes)
    priority = np.random.default_rng(5).permutation(n).astype(np.uint32)
    got = ctx.greedy_rows(idx, 0, KMER, 0.05, priority)
    check(got, orc.hits(0, 0.05), n, 0, priority)
    assert not np.array_equal(got[0], plain[0])
    few = (priority % 7).astype(np.uint32)   # many ties: the caller index decides
    check(ctx.greedy_rows(idx, 0, KMER, 0.05, few), orc.hits(0, 0.05), n, 0, few)


# ---- 6. more pairs than the hit buffer holds ----------------------------------------------------------------------------
def test_hit_buffer_overflow_runs_the_join_again(ctx):
    h, off = hit_overflow_collection()
    orc = Oracle(h, off, 24)
    hits = orc.hits(0, 0.05)
    assert len(hits) == 400 * 399 // 2 > max(65536, 403 * 64)
    got = ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    check(got, hits, 403, 0, sizes=orc.sizes)
    assert got[2]["join_attempts"] == 2 and got[2]["edges"] == len(hits) and got[2]["n_reps"] == 4 and len(got[1]) == 399


# ---- 7. a pair exactly on the threshold decides what happens down the chain ---------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_borderline_record_flips_the_outcome_down_a_chain(ctx, metric):
    """A - B share 30 of 100, B - C share 70, A - C share nothing; caller order A < B < C among unrelated sketches.  (B - C at 80, as
    first planned, is not possible: B has 100 hashes, 30 of them A's, and C must keep clear of A.)"""
    rng = np.random.default_rng(7)
    pool = np.unique(rng.integers(0, 1 << 24, size=3000))
    rng.shuffle(pool)
    fill = [np.sort(pool[300 + 100 * k: 400 + 100 * k]) for k in range(20)]
    a = pool[:100]
    b = np.concatenate([a[:30], pool[100:170]])
    c = np.concatenate([pool[100:170], pool[170:200]])
    parts = fill[:5] + [np.sort(a)] + fill[5:9] + [np.sort(b)] + fill[9:16] + [np.sort(c)] + fill[16:]
    A, B, Cc = 5, 10, 18
    h, off = csr(parts)
    n = len(parts)
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    for D, linked in ((float(np.nextafter(d0, 0.0)), False), (d0, False), (float(np.nextafter(d0, 1.0)), True)):   # strict <
        hits = orc.hits(metric, D)
        assert [t[:3] for t in gr.hit_tuples(hits)] == ([(A, B, 30)] if linked else []) + [(B, Cc, 70)]
        got = ctx.greedy_rows(idx, metric, KMER, D)
        check(got, hits, n, metric, sizes=orc.sizes)
        rep, links, st = got
        assert st["borderline"] >= 1 and st["borderline_kept"] == int(linked)
        assert (rep[A], rep[B], rep[Cc]) == ((A, A, Cc) if linked else (A, B, B))
        assert st["n_reps"] == n - 1


# ---- 8. more borderline records than their buffer holds -----------------------------------------------------------------
def test_borderline_overflow_runs_the_key_pass_again(ctx, monkeypatch):
    h, off = borderline_overflow_collection()
    _, d0 = ok.distance(80, 100, 100, 0, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "1")
    up = float(np.nextafter(d0, 1.0))
    got = ctx.greedy_rows(idx, 0, KMER, up)
    check(got, orc.hits(0, up), 600, 0, sizes=orc.sizes)
    st = got[2]
    assert st["border_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 300 and st["n_reps"] == 300 and st["rounds"] == 2
    got = ctx.greedy_rows(idx, 0, KMER, d0)
    check(got, orc.hits(0, d0), 600, 0, sizes=orc.sizes)
    st = got[2]
    assert st["border_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 0 and st["n_reps"] == 600 and st["rounds"] == 0
    assert len(got[1]) == 0
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "300")   # room for exactly all of them: one pass
    got = ctx.greedy_rows(idx, 0, KMER, up)
    check(got, orc.hits(0, up), 600, 0, sizes=orc.sizes)
    assert got[2]["border_attempts"] == 1 and got[2]["borderline"] == 300


# ---- 8b. both overflows in one call -------------------------------------------------------------------------------------
def test_hit_and_borderline_overflow_in_one_call(ctx, monkeypatch):
    """The hit overflow ends the first attempt before the borderline overflow is looked at; the key pass behind the second join
    overflows the borderline buffer and runs again."""
    h, off = both_overflows_collection()
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    for D, n_hits, kept in both_overflows_thresholds():
        hits = orc.hits(0, D)
        assert len(hits) == n_hits > max(65536, 420 * 64) and int(np.sum(hits["common"] == 80)) == kept
        got = ctx.greedy_rows(idx, 0, KMER, D)
        check(got, hits, 420, 0, sizes=orc.sizes)
        st = got[2]
        assert st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        assert st["n_reps"] == 21 - kept and len(got[1]) == 399 + kept


# ---- 9. every kernel of the join, both metrics, 36-bit hashes -----------------------------------------------------------
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
    got = ctx.greedy_rows(idx, metric, kmer, 0.05)
    rep, links = check(got, hits, n, metric, sizes=orc.sizes)
    gr.check_properties(gr.hit_tuples(hits), n, metric, rep, links, sizes=orc.sizes)
    st = got[2]
    assert st["edges"] >= len(hits) > len(links) > 0 and 1 < st["n_reps"] < n and st["rounds"] >= 2


# ---- 10. nothing to decide, and what is refused -------------------------------------------------------------------------
def test_empty_index_single_genome_and_no_pair(ctx):
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    rep, links, st = ctx.greedy_rows(none, 0, KMER, 0.05)
    assert len(rep) == 0 and len(links) == 0 and st["n_reps"] == 0 and st["join_attempts"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for D in (0.05, 1.0):
        rep, links, st = ctx.greedy_rows(one, 0, KMER, D)
        assert rep.tolist() == [0] and len(links) == 0 and st["n_reps"] == 1 and st["edges"] == 0 and st["rounds"] == 0
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h, off = csr(parts)
    orc = Oracle(h, off, 24)
    hits = orc.hits(0, 0.05)
    assert len(hits) == 0
    got = ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    check(got, hits, 500, 0, sizes=orc.sizes)
    assert got[0].tolist() == list(range(500)) and got[2]["n_reps"] == 500 and got[2]["rounds"] == 0 and len(got[1]) == 0


def raw_call(ctx, idx, opts, n, rep=True, links=True, n_links=True, stats=True):
    L = capi.lib()
    L.rk_greedy_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_uint64), C.POINTER(capi.GreedyStats)]
    rep_buf = np.zeros(n, dtype=np.uint32)
    out, n_out, st = C.c_void_p(), C.c_uint64(), capi.GreedyStats()
    rc = L.rk_greedy_rows(ctx._h, idx._h, C.byref(opts), None, rep_buf.ctypes.data if rep else None, C.byref(out) if links else None,
                          C.byref(n_out) if n_links else None, C.byref(st) if stats else None)
    if links:
        L.rk_free_host(out)
    return rc, int(n_out.value)


def test_arguments_that_are_refused(ctx):
    names, h, off, bits, wide, orc = collection("repeat")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for D in (1.5, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(capi.RkError) as e:
            ctx.greedy_rows(idx, 0, KMER, D)
        assert e.value.code == RK_ERR_ARG and "dense" in str(e.value)
    check(ctx.greedy_rows(idx, 0, KMER, 1.0), orc.hits(0, 1.0), n, 0, sizes=orc.sizes)   # the default -D 1.0 of alldist stays sparse
    assert raw_call(ctx, idx, capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1), n)[0] == RK_ERR_ARG   # triangle 0
    assert raw_call(ctx, idx, capi.DistOpts(1, 0, KMER, 32, 0.05, 0, 2), n)[0] == RK_ERR_ARG   # a row shard
    assert b"row shards" in capi.lib().rk_last_error(ctx._h)
    good = capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1)
    assert raw_call(ctx, idx, good, n, rep=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, links=False)[0] == RK_ERR_ARG
    assert raw_call(ctx, idx, good, n, n_links=False)[0] == RK_ERR_ARG
    rc, n_links = raw_call(ctx, idx, good, n, stats=False)   # stats is optional
    assert rc == 0 and n_links > 0
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = orc.built
        ctx.greedy_rows(ctx.index_import(postings, counts, 24, np.diff(off)), 0, KMER, 0.05)
    assert e.value.code == RK_ERR_ARG


def test_records_outside_the_key_are_refused(ctx):
    rng = np.random.default_rng(9)
    six = np.sort(np.unique(rng.integers(0, 1 << 24, size=20))[:6])
    one = np.sort(np.concatenate([six, six[:1], six[:1]]))   # eight hashes, one of them three times
    h, off = csr([one, one])
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 1 and hits["common"][0] > hits["size0"][0] + hits["size1"][0] - hits["common"][0]   # common > u
    with pytest.raises(capi.RkError) as e:
        ctx.greedy_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    assert e.value.code == RK_ERR_UNSUPPORTED and "common" in str(e.value)


def test_shards_of_a_sharded_build_are_refused(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.greedy_rows(parts[0], 0, KMER, 0.1)
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
    _, st = ctx.forest_rows(j, 0, KMER, 0.1)   # a forest accepts the join-only index: it holds the rows of shard 0
    assert st["edges"] > 0
    with pytest.raises(capi.RkError) as e:
        ctx.greedy_rows(j, 0, KMER, 0.1)
    assert e.value.code == RK_ERR_ARG and "join-only" in str(e.value)
    del j, parts, sk


# ---- 11. the host rule over the join's own hit list ---------------------------------------------------------------------
def test_greedy_hits_over_dist_rows_equals_greedy_rows(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    for metric in (0, 1):
        rep, links, st = ctx.greedy_rows(idx, metric, KMER, 0.05)
        hits = ctx.dist_rows(idx, None, 1, metric, KMER, 0.05)[0]
        assert len(hits) == st["edges"] - st["borderline"] + st["borderline_kept"]
        host_rep, host_links = capi.greedy_hits(hits, n, metric)
        assert np.array_equal(host_rep, rep) and len(links) == n - st["n_reps"]
        for f in capi.HIT_DTYPE.names:
            if f != "pad":
                assert np.array_equal(host_links[f], links[f]), f


# ---- 12. the tool -------------------------------------------------------------------------------------------------------
def test_tool_greedy_subcommand(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "ref.sketch")
    _, names, _, _ = ok.read_sketches32(os.path.join(GOLDEN, "dist", "ref.sketch"))
    assert len(set(names)) == len(names)
    n = len(names)
    number = {name: i for i, name in enumerate(names)}
    for metric in (0, 1):
        lines = open(os.path.join(GOLDEN, "dist", "alldist_M%d_D0.3.ref.txt" % metric)).read().splitlines()
        hits, dist_text = [], {}
        for line in lines:   # name[col] \t name[row] \t common|size0|size1 \t jorc \t dist  (the real reference's output)
            a, b, counts, _, dist = line.split("\t")
            hit = (number[b], number[a]) + tuple(int(x) for x in counts.split("|"))
            assert hit[0] < hit[1]
            hits.append(hit)
            dist_text[hit[:2]] = dist
        rep, links = gr.greedy(hits, n, metric)
        reps = [i for i in range(n) if rep[i] == i]
        assert 1 < len(reps) < n
        want = ""
        for k, r in enumerate(reps):
            cluster = [r] + [i for i in range(n) if rep[i] == r and i != r]
            for i in cluster:
                want += "%u\t%u\t%s\t%s\t%s\n" % (k, len(cluster), names[i], names[r], "0.000000" if i == r else dist_text[links[i][:2]])
        out, reps_file = tmp_path / ("g%d.txt" % metric), tmp_path / ("reps%d.txt" % metric)
        p = subprocess.run([TOOL, "greedy", "-i", "ref.sketch", "-D", "0.3", "-M", str(metric), "-o", out.name, "--reps", reps_file.name],
                           cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert out.read_text() == want, metric
        assert reps_file.read_text() == "".join(names[r] + "\n" for r in reps)
    p = subprocess.run([TOOL, "greedy", "-i", "ref.sketch", "-D", "0.3", "-o", "two.txt", "--gpus", "2"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"greedy runs on one GPU" in p.stderr and not (tmp_path / "two.txt").exists()
    p = subprocess.run([TOOL, "greedy", "-i", "ref.sketch", "-D", "1.5", "-o", "dense.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"must not exceed 1.0" in p.stderr
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"greedy -i" in p.stderr
