"""rk_cluster_rows: the single-linkage clusters of the self join against a Python union-find over the ORACLE's hit list
(ok.index_build32 + ok.index_dist32, triangle 1) -- label for label.  Every case says from the call's stats that it reached the
edge it is about (a retry, a borderline record, a kernel)."""
import subprocess

import numpy as np
import pytest

from _selfjoin_cases import (KMER, TOOL, Oracle, borderline_overflow_collection, both_overflows_collection, both_overflows_thresholds,
                             bridge_collection, csr, device_index, hit_overflow_collection, labels_of, permuted)
from oracle import oracle as ok
from rabbitkssd_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def check(labels, stats, want, n_hits=None):
    assert np.array_equal(labels, want)
    assert np.array_equal(labels[labels], labels) and np.all(labels <= np.arange(len(labels)))
    assert stats["n_clusters"] == len(np.unique(want))
    assert stats["borderline_kept"] <= stats["borderline"] <= stats["edges"]
    if n_hits is not None:   # nothing borderline: the device consumed exactly the oracle's pairs
        assert stats["edges"] - stats["borderline"] + stats["borderline_kept"] == n_hits


# ---- 1. a path: one component of diameter N - 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["identity", "permuted"])
def test_path_of_2000_genomes(ctx, order):
    n, m, step = 2000, 100, 5
    rng = np.random.default_rng(1)
    pool = np.unique(rng.integers(0, 1 << 28, size=step * n + m + 4000))[: step * (n - 1) + m]
    assert len(pool) == step * (n - 1) + m
    parts = [pool[step * i: step * i + m] for i in range(n)]   # neighbours share 95 of 100: d = -ln(0.95) / 20 = 0.00256; next but one 0.00527
    if order == "permuted":
        parts = permuted(parts, 11)
    h, off = csr(parts)
    orc = Oracle(h, off, 28)
    idx = device_index(ctx, h, off, 28)
    want, n_hits = orc.labels(0, 0.004)
    assert n_hits == n - 1 and np.all(want == 0)
    labels, st = ctx.cluster_rows(idx, 0, KMER, 0.004)
    check(labels, st, want, n_hits)
    assert st["edges"] == n - 1 and st["n_clusters"] == 1 and st["join_attempts"] == 1 and st["hook_attempts"] == 1
    want, n_hits = orc.labels(0, 0.002)
    assert n_hits == 0
    labels, st = ctx.cluster_rows(idx, 0, KMER, 0.002)
    check(labels, st, want, n_hits)
    assert st["edges"] == 0 and st["n_clusters"] == n and np.array_equal(labels, np.arange(n))


# ---- 2. a star and a bridge ---------------------------------------------------------------------------------------------
def test_star_of_3000_leaves(ctx):
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 24, size=140000))
    rng.shuffle(pool)
    hub, fresh = pool[:100], pool[100:]
    parts = [np.sort(hub)]
    for k in range(3000):   # a leaf: 60 of the hub's hashes and 40 of its own -- hub-leaf d = 0.0255, leaf-leaf ~0.05 (36 of 60 shared)
        parts.append(np.sort(np.concatenate([rng.choice(hub, size=60, replace=False), fresh[40 * k: 40 * k + 40]])))
    parts = permuted(parts, 12)
    h, off = csr(parts)
    orc = Oracle(h, off, 24)
    want, n_hits = orc.labels(0, 0.03)
    assert np.all(want == 0) and n_hits >= 3000
    labels, st = ctx.cluster_rows(device_index(ctx, h, off, 24), 0, KMER, 0.03)
    check(labels, st, want, n_hits)
    assert st["n_clusters"] == 1 and st["edges"] >= 3000


def test_two_cliques_bridged_by_the_two_largest_indices(ctx):
    h, off = bridge_collection(150, 3)
    n = len(off) - 1
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    want, n_hits = orc.labels(0, 0.07)
    assert np.all(want == 0)
    labels, st = ctx.cluster_rows(idx, 0, KMER, 0.07)
    check(labels, st, want, n_hits)
    assert st["n_clusters"] == 1
    want, n_hits = orc.labels(0, 0.05)   # without the bridge
    labels, st = ctx.cluster_rows(idx, 0, KMER, 0.05)
    check(labels, st, want, n_hits)
    assert st["n_clusters"] == 2 and labels[n - 1] != labels[n - 2]


# ---- 3. more pairs than the hit buffer holds ----------------------------------------------------------------------------
def test_hit_buffer_overflow_runs_the_join_again(ctx):
    h, off = hit_overflow_collection()
    orc = Oracle(h, off, 24)
    want, n_hits = orc.labels(0, 0.05)
    assert n_hits == 400 * 399 // 2 > max(65536, 403 * 64)
    labels, st = ctx.cluster_rows(device_index(ctx, h, off, 24), 0, KMER, 0.05)
    check(labels, st, want, n_hits)
    assert st["join_attempts"] == 2 and st["edges"] == n_hits and st["n_clusters"] == 4


# ---- 4. a pair exactly on the threshold ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_bridge_exactly_on_the_threshold(ctx, metric):
    h, off = bridge_collection(20, 5)
    n = len(off) - 1
    _, d0 = ok.distance(30, 100, 100, metric, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    want, n_hits = orc.labels(metric, d0)   # strict <: the bridge is not reported
    assert len(np.unique(want)) == 2
    labels, st = ctx.cluster_rows(idx, metric, KMER, d0)
    check(labels, st, want, n_hits)
    assert st["borderline"] >= 1 and st["borderline_kept"] == 0 and st["n_clusters"] == 2 and labels[n - 1] != labels[n - 2]
    up = float(np.nextafter(d0, 1.0))
    want, n_hits = orc.labels(metric, up)
    assert np.all(want == 0)
    labels, st = ctx.cluster_rows(idx, metric, KMER, up)
    check(labels, st, want, n_hits)
    assert st["borderline"] >= 1 and st["borderline_kept"] >= 1 and st["n_clusters"] == 1


# ---- 5. more borderline records than their buffer holds -----------------------------------------------------------------
def test_borderline_overflow_runs_the_hook_pass_again(ctx, monkeypatch):
    h, off = borderline_overflow_collection()
    _, d0 = ok.distance(80, 100, 100, 0, KMER)
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    up = float(np.nextafter(d0, 1.0))
    want, n_hits = orc.labels(0, up)
    assert n_hits == 300
    labels, st = ctx.cluster_rows(idx, 0, KMER, up)
    check(labels, st, want, n_hits)
    assert st["hook_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 300 and st["n_clusters"] == 300
    assert np.all(np.bincount(labels, minlength=600)[np.unique(labels)] == 2)
    want, n_hits = orc.labels(0, d0)
    assert n_hits == 0
    labels, st = ctx.cluster_rows(idx, 0, KMER, d0)
    check(labels, st, want, n_hits)
    assert st["hook_attempts"] == 2 and st["borderline"] == 300 and st["borderline_kept"] == 0 and st["n_clusters"] == 600
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "300")   # room for exactly all of them: one pass
    labels, st = ctx.cluster_rows(idx, 0, KMER, up)
    check(labels, st, orc.labels(0, up)[0], 300)
    assert st["hook_attempts"] == 1 and st["borderline"] == 300


# ---- 5b. both overflows in one call -------------------------------------------------------------------------------------
def test_hit_and_borderline_overflow_in_one_call(ctx, monkeypatch):
    """The hit overflow ends the first attempt before the borderline overflow is looked at; the hook pass behind the second join
    overflows the borderline buffer and runs again (its links stand: parent[] is not reset in between)."""
    h, off = both_overflows_collection()
    orc = Oracle(h, off, 24)
    idx = device_index(ctx, h, off, 24)
    monkeypatch.setenv("RK_CLUSTER_EDGE_CAP", "4")
    for D, want_hits, kept in both_overflows_thresholds():
        want, n_hits = orc.labels(0, D)
        assert n_hits == want_hits > max(65536, 420 * 64)
        labels, st = ctx.cluster_rows(idx, 0, KMER, D)
        check(labels, st, want, n_hits)
        assert st["join_attempts"] == 2 and st["hook_attempts"] == 2 and st["borderline"] == 10 and st["borderline_kept"] == kept
        assert st["n_clusters"] == 21 - kept


# ---- 6. every kernel of the join ----------------------------------------------------------------------------------------
def with_empties(names, h, off, at):
    """the collection with an empty sketch in front of every genome index in `at`"""
    sizes = np.diff(off).astype(np.int64).tolist()
    names = list(names)
    for k, i in enumerate(sorted(at)):
        sizes.insert(i + k, 0)
        names.insert(i + k, "syn/empty%d.fna" % k)
    new_off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(sizes)
    return names, h, new_off


_collections = {}


def collection(which):
    """(names, h, off, bits, wide, Oracle) of the named collection, built once per session and never changed.  This suite's own:
    "tiles" and "near" with empty sketches among their genomes, and "tree" on top"""
    if which not in _collections:
        wide, bits = False, 24
        if which == "tiles":     # 4,200 genomes and more than 4,000: tile records come with the build
            names, h, off = synth.clade_sketches(4200, 120, 24, strains_per_clade=10, seed=31, tiny=20)
            names, h, off = with_empties(names, h, off, (0, 777, 4100))
        elif which == "near":    # below 4,000 genomes, clades inside the window: the near-window kernel
            names, h, off = synth.clade_sketches(1200, 120, 24, strains_per_clade=10, seed=32)
            names, h, off = with_empties(names, h, off, (5, 600))
        elif which == "repeat":  # one sketch lists a hash twice: no sets, rk_dist_kernel
            names, h, off = synth.clade_sketches(64, 200, 24, strains_per_clade=10, seed=33)
            h = np.concatenate([h[:1], h])
            off = off.copy()
            off[1:] += np.uint64(1)
        elif which == "tree":    # species of 300: lineages >= 0.064 apart, inside a lineage <= 0.030
            names, h, off = synth.clade_sketches(900, 600, 24, strains_per_clade=300, seed=34)
        elif which == "wide":    # 36-bit hashes, the 64-bit layout
            names, h, off = synth.clade_sketches(1500, 150, 36, kmer_size=24, seed=15, wide=True)
            wide, bits = True, 36
        else:
            raise KeyError(which)
        if which != "repeat":
            order = synth.genome_order(len(names), "shuffled", seed=len(names))
            names, h, off = synth.permute_genomes(names, h, off, order)
        _collections[which] = (names, h, off, bits, wide, Oracle(h, off, bits, wide))
    return _collections[which]


@pytest.mark.parametrize("which,kernel,metric,D", [
    ("tiles", "rk_tile_kernel", 0, 0.05), ("tiles", "rk_tile_kernel", 1, 0.05),
    ("near", "rk_near_kernel", 0, 0.05), ("near", "rk_near_kernel", 1, 0.05),
    ("repeat", "rk_dist_kernel", 0, 0.05), ("repeat", "rk_dist_kernel", 1, 0.05),
    ("tree", None, 0, 0.05), ("tree", None, 1, 0.05),
    ("wide", None, 0, 0.05)])
def test_every_join_kernel(ctx, which, kernel, metric, D):
    names, h, off, bits, wide, orc = collection(which)
    kmer = 24 if wide else KMER
    idx = device_index(ctx, h, off, bits, wide)
    if kernel:
        assert ctx.dist_kernel_name(idx, None, 1, metric, kmer, D).startswith(kernel)
    want, n_hits = orc.labels(metric, D, kmer)
    labels, st = ctx.cluster_rows(idx, metric, kmer, D)
    check(labels, st, want, n_hits)
    assert st["edges"] >= n_hits > 0 and 1 < st["n_clusters"] < len(names)
    if which in ("tiles", "near"):
        assert np.all(labels[np.diff(off) == 0] == np.flatnonzero(np.diff(off) == 0))   # an empty sketch stays alone
    if which == "tree" and metric == 0:   # the lineages fall apart (3 species x 3 lineages), the sub-lineages hold
        assert st["n_clusters"] == 9 and np.all(np.bincount(labels)[np.unique(labels)] == 100)


# ---- 7. shards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [2, 3, 8])
def test_row_shards_fold_to_the_whole(ctx, step):
    names, h, off, bits, wide, orc = collection("tiles")
    idx = device_index(ctx, h, off, bits)
    want, n_hits = orc.labels(0, 0.05)
    folded = np.arange(len(names), dtype=np.uint32)
    edges = 0
    for first in range(step):
        labels, st = ctx.cluster_rows(idx, 0, KMER, 0.05, row_first=first, row_step=step, row_block=32)
        assert np.array_equal(labels[labels], labels) and np.all(labels <= np.arange(len(labels)))
        edges += st["edges"]
        folded = capi.cluster_merge(folded, labels)
    assert np.array_equal(folded, want) and edges == n_hits   # every pair on exactly one shard


@pytest.mark.parametrize("S", [2, 4])
def test_join_only_indexes_of_a_sharded_build_fold_to_the_whole(ctx, S):
    import torch
    names, h, off = synth.clade_sketches(1600, 120, 20, strains_per_clade=40, seed=53)
    names, h, off = synth.permute_genomes(names, h, off, synth.genome_order(len(names), "shuffled", seed=S))
    want, n_hits = Oracle(h, off, 20).labels(0, 0.1)
    assert n_hits > 1000
    sk = ctx.sketches_from_host(h, off)
    parts = [ctx.index_build_shard(sk, 20, d, S) for d in range(S)]
    with pytest.raises(capi.RkError) as e:   # one hash range of a sharded build: refused as rk_dist_rows refuses it
        ctx.cluster_rows(parts[0], 0, KMER, 0.1)
    assert e.value.code == -1
    sent = [p.shard_records(S) for p in parts]
    bufs = []
    for p, cnt in zip(parts, sent):
        b = torch.empty(max(1, sum(cnt) * 12), dtype=torch.uint8, device="cuda")
        p.shard_pack(b.data_ptr())
        bufs.append(b)
    torch.cuda.synchronize()
    folded = np.arange(len(names), dtype=np.uint32)
    edges = 0
    for d in range(S):   # the shards played in turn
        recv = torch.cat([bufs[r][12 * sum(sent[r][:d]): 12 * sum(sent[r][:d + 1])] for r in range(S)] + [torch.empty(1, dtype=torch.uint8, device="cuda")])
        torch.cuda.synchronize()
        j = ctx.index_join_shard(parts[d], recv.data_ptr(), sum(sent[r][d] for r in range(S)))
        labels, st = ctx.cluster_rows(j, 0, KMER, 0.1)
        edges += st["edges"]
        folded = capi.cluster_merge(folded, labels)
        del j
    assert np.array_equal(folded, want) and edges == n_hits
    del parts, sk


# ---- 8. dense reports and empty results ---------------------------------------------------------------------------------
def test_dense_report_single_genome_and_no_pair(ctx):
    names, h, off, bits, wide, orc = collection("near")
    n = len(names)
    idx = device_index(ctx, h, off, bits)
    labels, st = ctx.cluster_rows(idx, 0, KMER, 1.5)   # every pair is a hit: answered without a join
    assert np.all(labels == 0) and st["edges"] == 0 and st["join_attempts"] == 0 and st["n_clusters"] == 1
    # a row shard of a dense report: what rk_dist_rows reports for the same rows
    small = collection("repeat")
    sidx = device_index(ctx, small[1], small[2], 24)
    for first, step, block in ((1, 2, 8), (0, 2, 8), (3, 4, 16), (7, 8, 8), (1, 1, 10)):
        hits, _ = ctx.dist_rows(sidx, None, 1, 0, KMER, 1.5, row_first=first, row_step=step, row_block=block)
        labels, st = ctx.cluster_rows(sidx, 0, KMER, 1.5, row_first=first, row_step=step, row_block=block)
        assert np.array_equal(labels, labels_of(zip(hits["row"].tolist(), hits["col"].tolist()), 64)), (first, step, block)
        assert st["edges"] == 0
    one = device_index(ctx, np.array([3, 9, 27], dtype=np.uint32), np.array([0, 3], dtype=np.uint64), 12)
    for D in (0.05, 1.0, 1.5):
        labels, st = ctx.cluster_rows(one, 0, KMER, D)
        assert labels.tolist() == [0] and st["n_clusters"] == 1 and st["edges"] == 0
    none = device_index(ctx, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), 12)
    labels, st = ctx.cluster_rows(none, 0, KMER, 0.05)
    assert len(labels) == 0 and st["n_clusters"] == 0
    rng = np.random.default_rng(8)
    parts = [np.unique(rng.integers(0, 1 << 24, size=110))[:100] for _ in range(500)]   # unrelated: no reportable pair
    h2, off2 = csr(parts)
    want, n_hits = Oracle(h2, off2, 24).labels(0, 0.05)
    assert n_hits == 0
    labels, st = ctx.cluster_rows(device_index(ctx, h2, off2, 24), 0, KMER, 0.05)
    check(labels, st, want, 0)
    assert st["edges"] == 0 and st["n_clusters"] == 500
    # the default -D 1.0 of alldist stays sparse (`1.0 < 1.0` is false): every pair that shares a hash, nothing else
    want, n_hits = orc.labels(0, 1.0)
    labels, st = ctx.cluster_rows(idx, 0, KMER, 1.0)
    check(labels, st, want, n_hits)
    assert st["join_attempts"] >= 1 and 1 < st["n_clusters"] < n
    with pytest.raises(capi.RkError) as e:   # imported indexes have no self join
        postings, counts = small[5].built
        ctx.cluster_rows(ctx.index_import(postings, counts, 24, np.diff(small[2])), 0, KMER, 0.05)
    assert e.value.code == -1


# ---- 9. the tool --------------------------------------------------------------------------------------------------------
def cluster_text(names, labels):
    rep = np.unique(labels)
    number = {int(r): k for k, r in enumerate(rep)}
    size = np.bincount(labels, minlength=len(labels))
    order = np.lexsort((np.arange(len(labels)), labels))
    return "".join("%u\t%u\t%s\n" % (number[int(labels[i])], size[labels[i]], names[i]) for i in order)


def test_tool_cluster_subcommand(tmp_path):
    names, h, off, bits, wide, orc = collection("tiles")
    synth.write_sketch_file(str(tmp_path / "c.sketch"), 10, 6, 4, names, h, off)
    two = ["--gpus", "2"] + ([] if capi.lib().rk_device_count() >= 2 else ["--same-device"])
    for metric in (0, 1):
        want = cluster_text(names, orc.labels(metric, 0.05)[0])
        for extra in (["--gpus", "1"], two):   # (the first run writes .dict / .index: the second takes the sharded build)
            out = tmp_path / ("o%d%s.txt" % (metric, len(extra)))
            p = subprocess.run([TOOL, "cluster", "-i", "c.sketch", "-D", "0.05", "-M", str(metric), "-o", out.name] + extra,
                               cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert out.read_text() == want, (metric, extra)
    p = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"cluster -i" in p.stderr
