"""rk_forest_rows: the minimum spanning forest of the self join against tests/_forest_ref.py's Kruskal (exact rational weights)
over the ORACLE's hit list (ok.index_build32 + ok.index_dist32 / the 64-bit pair, triangle 1): the exact (row, col, common, size0,
size1) sequence, and dist / jorc bit for bit.  Every case says from the call's stats that it reached the edge it is about."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _forest_ref as fr
from _selfjoin_cases import (KMER, TOOL, Oracle, borderline_overflow_collection, both_overflows_collection, both_overflows_thresholds,
                             bridge_collection, collection, csr, device_index, hit_overflow_collection, identical, permuted,
                             tie_collection)
from conftest import GOLDEN
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def expect(hits, n, metric):
    """the reference forest of an oracle hit list: (hits in forest order, their jorc, their dist)"""
    value = {(int(r), int(c)): (float(j), float(d)) for r, c, j, d in zip(hits["row"], hits["col"], hits["jorc"], hits["dist"])}
    want = fr.kruskal(fr.hit_tuples(hits), n, metric)
    return want, [value[(h[0], h[1])][0] for h in want], [value[(h[0], h[1])][1] for h in want]


def check(edges, st, hits, n, metric):
    """edges and stats of one call (or of a fold) against the oracle's hit list; returns the reference forest"""
    want, jorc, dist = expect(hits, n, metric)
    assert fr.hit_tuples(edges) == want
    assert np.array_equal(edges["jorc"], np.array(jorc, dtype=np.float64)) and np.array_equal(edges["dist"], np.array(dist, dtype=np.float64))
    assert np.all(edges["row"] < edges["col"])
    if st is not None:
        assert st["n_trees"] == n - len(want)
        assert st["borderline_kept"] <= st["borderline"] <= st["edges"]
        assert st["edges"] - st["borderline"] + st["borderline_kept"] == len(hits)   # the device consumed exactly the oracle's pairs
    return want


# ---- 1. a path: Boruvka needs several rounds ----------------------------------------------------------------------------
def test_path_of_2048_genomes(ctx):
    n, m = 2048, 100
    rng = np.random.default_rng(1)
    share = rng.integers(50, 96, size=n - 1)   # neighbours share 50 .. 95 of 100: d <= -ln(0.5) / 20 = 0.0347
    pool = np.unique(rng.integers(0, 1 << 24, size=130000))
    rng.shuffle(pool)
    assert len(pool) >= m + int((m - share).sum())
    parts, used = [pool[:m]], m
    for i in range(n - 1):   # genome i + 1: share[i] hashes of genome i, the rest fresh
        fresh = m - int(share[i])
        parts.append(np.concatenate([rng.choice(parts[-1], size=int(share[i]), replace=False), pool[used: used + fresh]]))
        used += fresh
    parts = permuted([np.sort(p) for p in parts], 11)
    h, off = csr(parts)
    orc = Oracle(h, off, 24)
    edges, st = ctx.forest_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    want = check(edges, st, orc.hits(0, 0.05), n, 0)
    assert len(want) == n - 1 and st["n_trees"] == 1 and st["rounds"] >= 3 and st["join_attempts"] == 1 and st["border_attempts"] == 1


# ---- 2. every pair at distance 0 ----------------------------------------------------------------------------------------
def test_all_ties_give_the_star_of_genome_0(ctx):
    h, off = csr(permuted(identical(300, 2), 12))
    orc = Oracle(h, off, 24)
    hits = orc.hits(0, 0.05)
    assert len(hits) == 300 * 299 // 2 == 44850 and np.all(hits["dist"] == 0.0)
    edges, st = ctx.forest_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    check(edges, st, hits, 300, 0)
    assert st["edges"] == 44850 and st["n_trees"] == 1 and st["rounds"] >= 2
    assert edges["row"].tolist() == [0] * 299 and edges["col"].tolist() == list(range(1, 300))


# ---- 3. one ratio from different counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_equal_ratio_from_different_counts(ctx, metric):
    h, off = tie_collection(3)
    n = len(off) - 1
    orc = Oracle(h, off, 24)
    hits = orc.hits(metric, 0.06)
    triples = set(zip(hits["common"].tolist(), hits["size0"].tolist(), hits["size1"].tolist()))
    assert len(hits) == 6 * 4 and {(25, 50, 50), (26, 50, 51)} <= triples | {(c, b, a) for c, a, b in triples}
    assert {c for c, _, _ in triples} == {20, 25, 26}
    edges, st = ctx.forest_rows(device_index(ctx, h, off, 24), metric, KMER, 0.06)
    want = check(edges, st, hits, n, metric)
    assert len(want) == 6 * 3 and st["n_trees"] == n - 18
    if metric == 0:   # 26/75 first, then twelve edges at 1/3 from two different counts in (row, col) order
        assert [fr.ratio(w, 0) for w in want] == [fr.Fraction(26, 75)] * 6 + [fr.Fraction(1, 3)] * 12
        assert len({w[2] for w in want[6:]}) == 2 and [(w[0], w[1]) for w in want[6:]] == sorted((w[0], w[1]) for w in want[6:])


# ---- 4. bridges and a star ----------------------------------------------------------------------------------------------
def test_two_cliques_and_their_bridge(ctx):
    h, off = bridge_collection(150, 3)
    n = len(off) - 1
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    edges, st = ctx.forest_rows(idx, 0, KMER, 0.07)
    want = check(edges, st, orc.hits(0, 0.07), n, 0)
    assert st["n_trees"] == 1 and want[-1][:2] == (n - 2, n - 1)   # the bridge is the last edge of the dendrogram
    edges, st = ctx.forest_rows(idx, 0, KMER, 0.05)
    check(edges, st, orc.hits(0, 0.05), n, 0)
    assert st["n_trees"] == 2


def test_star_of_3000_leaves(ctx):
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=140000))
    rng.shuffle(pool)
    hub, spare = pool[:100], pool[100:]
    parts = [np.sort(hub)]
    for k in range(3000):   # a leaf: 60 of the hub's hashes and 40 of its own -- hub-leaf d = 0.0255, leaf-leaf ~0.05
        parts.append(np.sort(np.concatenate([rng.choice(hub, size=60, replace=False), spare[40 * k: 40 * k + 40]])))
    parts = permuted(parts, 12)
    h, off = csr(parts)
    orc = Oracle(h, off, 24)
    hits = orc.hits(0, 0.03)
    edges, st = ctx.forest_rows(device_index(ctx, h, off, 24), 0, KMER, 0.03)
    want = check(edges, st, hits, 3001, 0)
    assert len(want) == 3000 and st["n_trees"] == 1 and st["edges"] == len(hits) >= 3000


# ---- 5. more pairs than the hit buffer holds ----------------------------------------------------------------------------
def test_hit_buffer_overflow_runs_the_join_again(ctx):
    h, off = hit_overflow_collection()
    orc = Oracle(h, off, 24)
    hits = orc.hits(0, 0.05)
    assert len(hits) == 400 * 399 // 2 > max(65536, 403 * 64)
    edges, st = ctx.forest_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    want = check(edges, st, hits, 403, 0)
    assert st["join_attempts"] == 2 and st["edges"] == len(hits) and st["n_trees"] == 4 and len(want) == 399


# ---- 6. a pair exactly on the threshold, and one ulp either side --------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_bridge_on_the_threshold_and_one_ulp_either_side(ctx, metric):
    h, off = bridge_collection(20, 5)
    n = len(off) - 1
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    for D, bridged in ((float(np.nextafter(d0, 0.0)), False), (d0, False), (float(np.nextafter(d0, 1.0)), True)):   # strict <
        hits = orc.hits(metric, D)
        edges, st = ctx.forest_rows(idx, metric, KMER, D)
        want = check(edges, st, hits, n, metric)
        assert st["borderline"] >= 1 and st["borderline_kept"] == int(bridged) and st["n_trees"] == (1 if bridged else 2)
        assert ((n - 2, n - 1) in [w[:2] for w in want]) == bridged


# ---- 7. more borderline records than their buffer holds -----------------------------------------------------------------
def test_borderline_overflow_runs_the_key_pass_again(ctx, monkeypatch):
    h, off = borderline_overflow_collection()
    _, d0 = ok.distance(80, 100, 100, 0, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "1")
    up = float(np.nextafter(d0, 1.0))
    edges, st = ctx.forest_rows(idx, 0, KMER, up)
    want = check(edges, st, orc.hits(0, up), 600, 0)
    assert st["border_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 300 and len(want) == 300 and st["rounds"] == 0
    edges, st = ctx.forest_rows(idx, 0, KMER, d0)
    check(edges, st, orc.hits(0, d0), 600, 0)
    assert st["border_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 0 and len(edges) == 0 and st["n_trees"] == 600
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "300")   # room for exactly all of them: one pass
    edges, st = ctx.forest_rows(idx, 0, KMER, up)
    check(edges, st, orc.hits(0, up), 600, 0)
    assert st["border_attempts"] == 1 and st["borderline"] == 300


# ---- 7b. both overflows in one call -------------------------------------------------------------------------------------
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
        edges, st = ctx.forest_rows(idx, 0, KMER, D)
        check(edges, st, hits, 420, 0)
        assert st["join_attempts"] == 2 and st["border_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        assert len(edges) == 399 + kept and st["n_trees"] == 21 - kept


# ---- 8. every kernel of the join, both metrics, 36-bit hashes -----------------------------------------------------------
@pytest.mark.parametrize("which,kernel,metric", [
    ("tiles", "rk_tile_kernel", 0), ("tiles", "rk_tile_kernel", 1), ("near", "rk_near_kernel", 0), ("near", "rk_near_kernel", 1),
    ("repeat", "rk_dist_kernel", 0), ("repeat", "rk_dist_kernel", 1), ("wide", None, 0), ("wide", None, 1)])
def test_every_join_kernel_both_metrics_and_wide_hashes(ctx, which, kernel, metric):
    names, h, off, bits, wide, orc = collection(which)
    kmer = 24 if wide else KMER
    idx = device_index(ctx, h, off, bits, wide)
    if kernel:
        assert ctx.dist_kernel_name(idx, None, 1, metric, kmer, 0.05).startswith(kernel)
    hits = orc.hits(metric, 0.05, kmer)
    edges, st = ctx.forest_rows(idx, metric, kmer, 0.05)
    want = check(edges, st, hits, len(names), metric)
    assert st["edges"] >= len(hits) > len(want) > 0 and 1 < st["n_trees"] < len(names) and st["rounds"] >= 2


# ---- 9. shards ----------------------------------------------------------------------------------------------------------
def test_three_row_shards_fold_to_the_whole(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    hits = orc.hits(0, 0.05)
    whole, st = ctx.forest_rows(idx, 0, KMER, 0.05)
    check(whole, st, hits, n, 0)
    folded = np.zeros(0, dtype=capi.HIT_DTYPE)
    consumed = 0
    for first in range(3):
        part, st = ctx.forest_rows(idx, 0, KMER, 0.05, row_first=first, row_step=3, row_block=32)
        assert 0 < len(part) < len(whole) and st["n_trees"] == n - len(part)
        consumed += st["edges"] - st["borderline"] + st["borderline_kept"]
        folded = capi.forest_merge(folded, part, n, 0)
    assert consumed == len(hits)   # every pair on exactly one shard
    check(folded, None, hits, n, 0)
    for f in capi.HIT_DTYPE.names:
        assert np.array_equal(folded[f], whole[f]), f


def test_join_only_indexes_of_a_two_shard_build_fold_to_the_whole(ctx):
    import torch
    S = 2
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=S))
    n = len(names)
    hits = Oracle(h, off, 20).hits(0, 0.1)
    assert len(hits) > 1000
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.forest_rows(parts[0], 0, KMER, 0.1)
    assert e.value.code == -1
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    folded = np.zeros(0, dtype=capi.HIT_DTYPE)
    consumed = 0
    for d in range(S):   # the shards played in turn
        recv = torch.cat([bufs[r][12 * sum(sent[r][:d]): 12 * sum(sent[r][:d + 1])] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        j = ctx.index_join_shard(parts[d], recv.data_ptr(), sum(sent[r][d] for r in range(S)))
        part, st = ctx.forest_rows(j, 0, KMER, 0.1)
        consumed += st["edges"] - st["borderline"] + st["borderline_kept"]
        folded = capi.forest_merge(folded, part, n, 0)
        del j
    assert consumed == len(hits)
    check(folded, None, hits, n, 0)
    del parts, sk


# ---- 10. the cut --------------------------------------------------------------------------------------------------------
def test_cut_equals_cluster_rows_at_every_threshold(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    edges, st = ctx.forest_rows(idx, 0, KMER, 0.05)
    check(edges, st, orc.hits(0, 0.05), n, 0)
    for t in (0.005, 0.01, 0.02, 0.035, 0.05):
        hits = orc.hits(0, t)
        want = np.array(fr.components(zip(hits["row"].tolist(), hits["col"].tolist()), n), dtype=np.uint32)
        cut = capi.forest_cut(edges, n, t)
        labels, _ = ctx.cluster_rows(idx, 0, KMER, t)
        assert np.array_equal(cut, want) and np.array_equal(labels, want), t
    assert 1 < len(np.unique(capi.forest_cut(edges, n, 0.05))) < len(np.unique(capi.forest_cut(edges, n, 0.005))) < n


# ---- 11. nothing to span, and what is refused ---------------------------------------------------------------------------
def test_empty_index_single_genome_and_no_pair(ctx):
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    edges, st = ctx.forest_rows(none, 0, KMER, 0.05)
    assert len(edges) == 0 and st["n_trees"] == 0 and st["join_attempts"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for D in (0.05, 1.0):
        edges, st = ctx.forest_rows(one, 0, KMER, D)
        assert len(edges) == 0 and st["n_trees"] == 1 and st["edges"] == 0 and st["rounds"] == 0
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h, off = csr(parts)
    hits = Oracle(h, off, 24).hits(0, 0.05)
    assert len(hits) == 0
    edges, st = ctx.forest_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    check(edges, st, hits, 500, 0)
    assert st["n_trees"] == 500 and st["rounds"] == 0


def test_dense_report_and_other_arguments_are_refused(ctx):
    import ctypes as C
    names, h, off, bits, wide, orc = collection("repeat")
    idx = device_index(ctx, h, off, bits)
    for D in (1.5, float(np.nextafter(1.0, 2.0))):
        with pytest.raises(capi.RkError) as e:   # every pair a hit: a forest over pairs that share nothing is not offered
            ctx.forest_rows(idx, 0, KMER, D)
        assert e.value.code == -1 and "dense" in str(e.value)
    edges, st = ctx.forest_rows(idx, 0, KMER, 1.0)   # the default -D 1.0 of alldist stays sparse: every pair that shares a hash
    check(edges, st, orc.hits(0, 1.0), len(names), 0)
    L = capi.lib()
    L.rk_forest_rows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.DistOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                 C.POINTER(capi.ForestStats)]
    out, n_out = C.c_void_p(), C.c_uint64()
    opts = capi.DistOpts(0, 0, KMER, 0, 0.05, 0, 1)   # triangle 0
    assert L.rk_forest_rows(ctx._h, idx._h, C.byref(opts), C.byref(out), C.byref(n_out), None) == -1
    opts = capi.DistOpts(1, 0, KMER, 0, 0.05, 0, 1)
    assert L.rk_forest_rows(ctx._h, idx._h, C.byref(opts), None, C.byref(n_out), None) == -1
    assert L.rk_forest_rows(ctx._h, idx._h, C.byref(opts), C.byref(out), None, None) == -1
    assert L.rk_forest_rows(ctx._h, idx._h, C.byref(opts), C.byref(out), C.byref(n_out), None) == 0 and n_out.value > 0   # stats is optional
    L.rk_free_host(out)
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = orc.built
        ctx.forest_rows(ctx.index_import(postings, counts, 24, np.diff(off)), 0, KMER, 0.05)
    assert e.value.code == -1


# ---- 12. the tool -------------------------------------------------------------------------------------------------------
def test_tool_forest_subcommand(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "dist", "ref.sketch"), tmp_path / "ref.sketch")
    _, names, _, _ = ok.read_sketches32(os.path.join(GOLDEN, "dist", "ref.sketch"))
    assert len(set(names)) == len(names)
    number = {name: i for i, name in enumerate(names)}
    two = ["--gpus", "2", "--same-device"]
    for metric in (0, 1):
        lines = open(os.path.join(GOLDEN, "dist", "alldist_M%d_D0.3.ref.txt" % metric)).read().splitlines(keepends=True)
        line_of, hits = {}, []
        for line in lines:   # name[col] \t name[row] \t common|size0|size1 \t jorc \t dist  (the real reference's output)
            a, b, counts = line.split("\t")[:3]
            hit = (number[b], number[a]) + tuple(int(x) for x in counts.split("|"))
            assert hit[0] < hit[1]
            hits.append(hit)
            line_of[hit[:2]] = line
        want = "".join(line_of[w[:2]] for w in fr.kruskal(hits, len(names), metric))
        assert 0 < want.count("\n") < len(lines)
        for extra in (["--gpus", "1"], two):   # (the first run writes .dict / .index: the second takes the sharded build)
            out = tmp_path / ("f%d%s.txt" % (metric, len(extra)))
            p = subprocess.run([TOOL, "forest", "-i", "ref.sketch", "-D", "0.3", "-M", str(metric), "-o", out.name] + extra,
                               cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert out.read_text() == want, (metric, extra)
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"forest -i" in p.stderr
